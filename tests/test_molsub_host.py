"""No GPU: the definition of the graph substructure match (include/mdt_hip.h, mdt_sub_match) on its reference
(tests/molsub_ref.py) -- containment whatever the spelling, the agreed pairs, rows that are no molecule, the step cap -- and the
plumbing: C export and argument checks, op schema and shape inference, the refusals, the launch order of the screening call with
``require`` / ``forbid`` on a recording library, the cache of SubstructureSet and what the docstrings promise."""
import contextlib
import inspect
import os
import re

import pytest
import torch

import molkey_ref as K
import molsub_ref as B
import smiles_ref as S
from conftest import ROOT
import moleculediffusiontransformer_amd as M
from moleculediffusiontransformer_amd import generative as G, ops, runtime as rt

CAP_PATTERN = "C.C.C.C.C.C.CN"


@pytest.fixture(scope="module")
def spelled():
    return K.random_spellings()


# ---------------------------------------------------------------------------------------------------------------------
# the definition on the reference
# ---------------------------------------------------------------------------------------------------------------------
def test_every_spelling_of_a_graph_contains_every_spelling_of_itself(spelled):
    asked = 0
    for g, sp in spelled:
        small = [s for s in sp if len(s) <= B.MAX_WIDTH]
        for p in small[:2]:
            for t in sp:
                assert B.string_match(p, t)[0] == B.MATCH, (p, t)
                asked += 1
    assert asked > 2000


def test_the_verdict_does_not_depend_on_the_spelling_and_the_cap_hides_nothing_in_the_pools(spelled):
    """The condition of the cap: over random_spellings() and the 27 patterns the cap was chosen on, no pair is undecided and no
    root takes more than a few hundred steps (the prototype: 18; a molecule in a spelling of itself: 150)."""
    worst = undecided = 0
    for g, sp in spelled:
        for p in B.PATTERNS:
            results = [B.string_match(p, t) for t in sp]
            assert len({v for v, _ in results}) == 1, (p, sp)
            undecided += sum(v == B.UNDECIDED for v, _ in results)
            worst = max([worst] + [s for _, s in results])
    own = 0
    for g, sp in spelled:
        if len(sp[0]) <= B.MAX_WIDTH:
            verdict, steps = B.string_match(sp[0], sp[-1])
            undecided += verdict == B.UNDECIDED
            own = max(own, steps)
    print("most steps of a root: %d over the patterns, %d for a molecule in itself; %d undecided" % (worst, own, undecided))
    assert undecided == 0 and worst <= 300 and own <= 300


AGREED = [("CO", "OCC", True), ("C=O", "CC(=O)O", True), ("C=O", "CCO", False), ("C1CC1", "CCC", False), ("CCC", "C1CC1", True),
          ("c1ccccc1", "C1=CC=CC=C1", False), ("cc", "CC", False), ("cc", "c1ccccc1", True), ("*", "C", True), ("*", "[Na+].[Cl-]", True),
          ("*", "c1ccccc1", True), ("[NH3+]", "C[NH3+]", True), ("[NH3+]", "CN", False), ("[N]", "CN", True), ("N", "C[NH3+]", True),
          ("C.C", "CC", True), ("C.C", "C", False), ("C.C", "C.N", False), ("C(C1)1", "C1CC1", True), ("C(C1)1", "C=C", False),
          ("[CH4]", "C", False), ("C", "[CH4]", True), ("CC(C)C", "CCCC", False), ("CCCC", "CC(C)C", False), ("C#N", "N#CC#N", True),
          ("C1CC1.C1CC1", "C1CC1", False), ("C1CC1.C1CC1", "C1CC1CC1CC1", True)]


@pytest.mark.parametrize("pattern,target,inside", AGREED)
def test_agreed_pairs(pattern, target, inside):
    assert B.contains(pattern, target) is inside


def test_the_order_of_cc_and_the_bond_written_from_the_later_atom():
    assert K.graph("cc")[3] == [(0, 1, 5)] and K.graph("CC")[3] == [(0, 1, 1)]
    assert any(a > b for a, b, _ in K.graph("C(C1)1")[3])                   # the scan can write a > b


def test_rows_that_are_no_molecule_match_nothing_and_are_decided():
    for s in [""] + [s for s, _ in S.MALFORMED_TABLE + S.OVERVALENT_TABLE]:
        for p in ("*", "C", "C=O"):
            assert B.string_match(p, s[:64]) == (B.NONE, 0), (p, s)
            if len(s) <= 32:
                assert B.string_match(s, "CC(=O)O") == (B.NONE, 0), s       # ... and as a pattern is in nothing
    c = K.descriptor("C")
    two = (2, [c, c], 1, [(0, 1, 1)])
    assert B.match_arrays(*two, *two)[0] == B.MATCH
    for n, nb, bonds in ((3, 1, [(0, 3, 1)]), (9, 0, []), (2, 9, []), (-1, 0, []), (2, -1, []), (0, 0, [])):
        assert B.match_arrays(n, [c] * 8, nb, bonds, 1, [c], 0, [], width=8) == (B.NONE, [])           # as a target
        assert B.match_arrays(4, [c] * 4, 0, [], n, [c] * 8, nb, bonds, p_width=8) == (B.NONE, [])      # as a pattern


def test_the_cap():
    verdict, steps = B.string_match(CAP_PATTERN, "C" * 62 + ".N")
    assert (verdict, steps) == (B.UNDECIDED, 4096) and B.MAX_STEPS == 4096   # some root ran into the cap, none succeeded
    assert B.string_match(CAP_PATTERN, "C" * 61 + "CN")[0] == B.MATCH
    assert B.string_match("C.CN", "C" * 62 + ".N") == (B.NONE, 61)          # a small one of the same kind is decided: no C next to N
    assert B.flag(0, 1, 1, 0) == B.flag(0, 1, 0, 1) == 128 and B.flag(0, 1, 0, 0) == 0      # undecided counts against, both ways


# ---------------------------------------------------------------------------------------------------------------------
# header, library, binding
# ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_the_library_exports_the_new_symbol():
    hdr = open(os.path.join(ROOT, "include", "mdt_hip.h")).read()
    lib = rt.load_library()
    assert re.search(r"\bint mdt_sub_match\s*\(", hdr) and "mdt_sub_match" in rt.SYMBOLS and hasattr(lib, "mdt_sub_match")
    assert len(rt.SYMBOLS["mdt_sub_match"][1]) == 18
    assert int(re.search(r"#define MDT_ABI_VERSION (\d+)", hdr).group(1)) == rt.ABI_VERSION == 5 == lib.mdt_abi_version()
    assert int(re.search(r"#define MDT_SUB_MAX_PATTERNS (\d+)", hdr).group(1)) == rt.SUB_MAX_PATTERNS == G.MAX_SUB_PATTERNS == B.MAX_PATTERNS
    assert int(re.search(r"#define MDT_SUB_MAX_WIDTH (\d+)", hdr).group(1)) == rt.SUB_MAX_WIDTH == G.MAX_SUB_LENGTH == B.MAX_WIDTH
    assert int(re.search(r"#define MDT_SUB_MAX_STEPS (\d+)", hdr).group(1)) == rt.SUB_MAX_STEPS == B.MAX_STEPS == 4096
    assert int(re.search(r"MDT_SCREEN_SUBSTRUCTURE = (\d+)", hdr).group(1)) == rt.SCREEN_SUBSTRUCTURE == B.SUBSTRUCTURE == 128
    for phrase in ("not SMARTS", "not RDKit's HasSubstructMatch", "no implicit hydrogens", "no aromaticity perception", "no stereo",
                   "does not depend on how target or pattern is spelled", "undecided can depend on the spelling",
                   "no pre-filter", "no mapping is", "subgraph monomorphism"):
        assert phrase in " ".join(hdr.replace(" * ", " ").split()), phrase
    assert "k_molsub.hip" in [s for s, _ in __import__("moleculediffusiontransformer_amd.build", fromlist=["SOURCES"]).SOURCES]
    src = open(os.path.join(ROOT, "moleculediffusiontransformer_amd", "csrc", "k_molsub.hip")).read()
    assert "sub_root_search(" in src and "mdt_molsub.h" in src               # the kernel runs the search the host check runs


def test_entry_point_refuses_bad_arguments_before_any_launch():
    lib = rt.load_library()

    def sub(L=32, R_=5, LP=8, P=3, need=1, ban=2, p=8, pp=8, out=8, flags=8):
        return lib.mdt_sub_match(p, p, p, p, L, R_, pp, pp, pp, pp, LP, P, need, ban, out, out, flags, 0)
    for kw, what in ((dict(L=0), b"L <= 64"), (dict(L=65), b"L <= 64"), (dict(R_=-1), b"R >= 0"), (dict(LP=0), b"LP <= 32"),
                     (dict(LP=33), b"LP <= 32"), (dict(P=0), b"P <= 32"), (dict(P=33), b"P <= 32"), (dict(need=8), b"below P"),
                     (dict(ban=8), b"below P"), (dict(need=3, ban=2), b"overlap"), (dict(p=0), b"null"), (dict(pp=0), b"null"),
                     (dict(out=0), b"null")):
        assert sub(**kw) == 2, kw
        assert what in lib.mdt_last_error(), (kw, lib.mdt_last_error())
    assert sub(R_=0) == 0 and sub(R_=0, p=0, pp=0, out=0, flags=0) == 0      # nothing to do: nothing is launched, nothing is read
    assert sub(R_=0, P=32, need=0x80000000, ban=0x7FFFFFFF) == 0            # every bit of 32 patterns
    assert sub(R_=0, P=0) != 0 and sub(R_=0, need=1, ban=1) != 0             # ... but a bad argument is still one


def vocabulary():
    return M.SmilesVocabulary([None] + S.CHARS)


def test_op_schema_and_shape_inference():
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert str(torch.ops.mdt.sub_match.default._schema) == \
        ("mdt::sub_match(Tensor natoms, Tensor atoms, Tensor nbonds, Tensor bonds, Tensor p_natoms, Tensor p_atoms, Tensor p_nbonds, "
         "Tensor p_bonds, SymInt need, SymInt ban) -> (Tensor, Tensor, Tensor)")
    with FakeTensorMode():
        n, rows = torch.empty(15, dtype=torch.int32), torch.empty(15, 40, dtype=torch.int32)
        pn, prows = torch.empty(3, dtype=torch.int32), torch.empty(3, 9, dtype=torch.int32)
        out = torch.ops.mdt.sub_match(n, rows, n, rows, pn, prows, pn, prows, 1, 2)
        assert [(tuple(t.shape), t.dtype) for t in out] == [((15,), torch.int32), ((15,), torch.int32), ((15,), torch.uint8)]
    n, rows = torch.zeros(3, dtype=torch.int32), torch.zeros(3, 4, dtype=torch.int32)       # no CPU implementation behind the op
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        torch.ops.mdt.sub_match(n, rows, n, rows, n, rows, n, rows, 0, 0)


# ---------------------------------------------------------------------------------------------------------------------
# on a recording library: launch order, refusals with nothing launched, the cache
# ---------------------------------------------------------------------------------------------------------------------
class Recorder:
    """Stands for libmdt_hip.so: every launch is appended to ``log``."""

    def __init__(self):
        self.log = []

    def __getattr__(self, name):
        if not name.startswith("mdt_"):
            raise AttributeError(name)
        return lambda *a: self.log.append((name,) + a) or 0


@pytest.fixture
def rec(monkeypatch):
    rec = Recorder()
    monkeypatch.setattr(rt, "load_library", lambda *a, **k: rec)
    monkeypatch.setattr(rt, "current_stream", lambda: 0)
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    monkeypatch.setattr(ops, "_hip", lambda *t: torch.device("cpu"))         # (the device guard: there is no device here)
    return rec


class Fwd:
    max_length = 24

    def __init__(self, rec):
        self.rec = rec

    def sample(self, data, device, **k):
        self.rec.log.append(("forward_sample", data, k))
        return torch.zeros(data.shape[0], 1, 24)


N_, G_, K_, L_, n_ = 5, 3, 2, 16, 12
PATTERN_GRAPHS = ["mdt_tokens_compact", "mdt_mol_graph"]                    # SubstructureSet.on(), the first time per device


def names(rec):
    return [e[0] for e in rec.log]


def test_launch_order_of_the_screening_call_with_require_and_forbid(rec):
    tok, cond, v = torch.ones(N_ * G_, L_, dtype=torch.long), torch.zeros(G_, n_), vocabulary()
    known = M.KnownSet(torch.ones(4, L_, dtype=torch.long), L_)
    need, bad = M.SubstructureSet(["C=O", "N"], v), M.SubstructureSet(["C#N", "OO", "c1ccccc1"], v)
    run = lambda **kw: (rec.log.clear(), M.screen_tokens_diverse(Fwd(rec), tok, cond, "cpu", N_, K_, **kw), names(rec)[3:])[2]  # noqa: E731
    # require alone: the candidates' graph once, the patterns' graphs the first time only, one match, today's selection
    for again in (False, True):
        assert run(vocabulary=v, require=need) == ["mdt_smiles_check", "mdt_mol_graph"] + ([] if again else PATTERN_GRAPHS) + \
            ["mdt_sub_match", "mdt_screen_select_reject"]
    check, graph, sub, select = rec.log[3:]
    assert sub[1:7] == (graph[8], graph[9], graph[10], graph[11], L_, N_ * G_) and sub[11:15] == (3, 2, 0b11, 0) and len(sub) == 1 + 18
    assert sub[7:11] == tuple(t.data_ptr() for t in need.on("cpu")) and sub[17] != 0
    assert select[13] not in (0, check[8])                                   # reject = the check's status | the flags
    # forbid alone, then both: the patterns concatenated, require first, the narrower set padded
    assert run(vocabulary=v, forbid=bad)[-4:] == PATTERN_GRAPHS + ["mdt_sub_match", "mdt_screen_select_reject"]
    assert rec.log[-2][11:15] == (8, 3, 0, 0b111)
    assert run(vocabulary=v, require=need, forbid=bad) == ["mdt_smiles_check", "mdt_mol_graph", "mdt_sub_match", "mdt_screen_select_reject"]
    assert rec.log[-2][11:15] == (8, 5, 0b11, 0b11100)
    # lists of strings are wrapped (and their graphs computed) per call
    assert run(vocabulary=v, require=["CO"], forbid=["N", "O"], min_distance=2) == \
        ["mdt_smiles_check", "mdt_mol_graph"] + PATTERN_GRAPHS * 2 + ["mdt_sub_match", "mdt_screen_select_diverse_reject"]
    assert rec.log[-2][11:15] == (2, 3, 0b1, 0b110)
    # with graph identity and the similarity threshold: ONE mdt_mol_graph over the candidates feeds the key, the match, the fingerprint
    assert run(vocabulary=v, identity="graph", require=need, forbid=bad, max_similarity=0.5) == \
        ["mdt_smiles_check", "mdt_mol_graph", "mdt_mol_key", "mdt_key_flags", "mdt_sub_match", "mdt_mol_fp", "mdt_screen_select_similar"]
    graph, sub, fp = rec.log[4], rec.log[7], rec.log[8]
    assert sub[1:5] == graph[8:12] == fp[1:5]
    assert run(vocabulary=v, known_tokens=known, identity="graph", forbid=bad, max_known_similarity=0.7, min_novelty=2) == \
        ["mdt_smiles_check", "mdt_mol_graph", "mdt_mol_key", "mdt_mol_graph", "mdt_mol_key", "mdt_key_flags", "mdt_sub_match", "mdt_mol_fp",
         "mdt_mol_graph", "mdt_mol_fp", "mdt_fp_nearest", "mdt_edit_nearest", "mdt_screen_select_diverse_reject"]
    assert [e[4] for e in rec.log if e[0] == "mdt_mol_graph"] == [N_ * G_, len(known), len(known)]     # the candidates' graph: once
    # with both at None the launches are those made before the keywords existed
    parent = {(): ["mdt_screen_select"], (("vocabulary", v),): ["mdt_smiles_check", "mdt_screen_select_reject"],
              (("min_distance", 2),): ["mdt_screen_select_diverse"],
              (("vocabulary", v), ("min_distance", 2)): ["mdt_smiles_check", "mdt_screen_select_diverse_reject"],
              (("known_tokens", known), ("min_novelty", 2)): ["mdt_edit_nearest", "mdt_screen_select_diverse"],
              (("vocabulary", v), ("identity", "graph")): ["mdt_smiles_check", "mdt_mol_graph", "mdt_mol_key", "mdt_key_flags",
                                                          "mdt_screen_select_reject"],
              (("vocabulary", v), ("max_similarity", 0.5)): ["mdt_smiles_check", "mdt_mol_graph", "mdt_mol_fp", "mdt_screen_select_similar"]}
    for kw, want in parent.items():
        logs = []
        for extra in (dict(), dict(require=None, forbid=None)):
            assert run(**dict(kw), **extra) == want, kw
            logs.append([(e[0], len(e), tuple(a for a in e[1:] if isinstance(a, int) and a < 4096)) for e in rec.log])
        assert logs[0] == logs[1]
    # the public call
    rec.log.clear()
    match, undecided, status, position = M.has_substructure(tok.to(torch.int16), bad, v, "cpu")
    assert names(rec) == ["mdt_tokens_compact", "mdt_mol_graph", "mdt_sub_match"] and rec.log[2][5:7] == (L_, N_ * G_)
    assert rec.log[2][11:15] == (8, 3, 0, 0)
    assert match.shape == undecided.shape == (N_ * G_, 3) and match.dtype == undecided.dtype == torch.bool
    assert all(t.dtype == torch.int64 and t.shape == (N_ * G_,) for t in (status, position))
    rec.log.clear()
    assert M.has_substructure(tok, ["C", "CC(=O)O"], v, "cpu")[0].shape == (N_ * G_, 2)
    assert names(rec) == ["mdt_tokens_compact", "mdt_mol_graph"] + PATTERN_GRAPHS + ["mdt_sub_match"] and rec.log[-1][11:13] == (7, 2)


def test_screen_candidates_forwards_the_keywords_only_when_set(rec, monkeypatch):
    seen = {}

    class Inv:
        max_length = 32

        def sample_tokens(self, seq, device, **k):
            return torch.ones(seq.shape[0], 32, dtype=torch.long)
    monkeypatch.setattr(G, "screen_tokens", lambda *a, **k: seen.update(plain=k) or "plain")
    monkeypatch.setattr(G, "screen_tokens_diverse", lambda *a, **k: seen.update(diverse=k) or "diverse")
    cond, v = torch.zeros(2, 12), vocabulary()
    need = M.SubstructureSet(["C=O"], v)
    assert M.screen_candidates(Inv(), "fwd", cond, "dev", 3, 2, vocabulary=v, require=need) == "diverse"
    assert seen["diverse"] == dict(min_distance=1, min_novelty=1, vocabulary=v, require=need)
    assert M.screen_candidates(Inv(), "fwd", cond, "dev", 3, 2, vocabulary=v, forbid=["C#N"], require=None) == "diverse"
    assert seen["diverse"] == dict(min_distance=1, min_novelty=1, vocabulary=v, forbid=["C#N"])
    assert M.screen_candidates(Inv(), "fwd", cond, "dev", 3, 2, require=None, forbid=None) == "plain"
    assert seen["plain"] == dict()                                           # as without the keywords
    assert list(inspect.signature(M.screen_candidates).parameters)[-1] == "screen_tokens_kwargs"
    assert rec.log == []


def test_refusals_come_before_anything_is_launched(rec):
    fwd, v = Fwd(rec), vocabulary()
    tok, cond = torch.ones(N_ * G_, L_, dtype=torch.long), torch.zeros(G_, n_)
    wide = torch.ones(N_ * G_, 65, dtype=torch.long)
    div = lambda t=tok, **kw: M.screen_tokens_diverse(fwd, t, cond, "cpu", N_, K_, **kw)  # noqa: E731

    class Inv:
        max_length = 65

        def sample_tokens(self, *a, **k):
            raise AssertionError("sampled")
    for call, what in (
            (lambda: div(require=["C"]), "give a vocabulary"),
            (lambda: div(forbid=["C"]), "give a vocabulary"),
            (lambda: div(wide, vocabulary=v, require=["C"]), "at most 64"),
            (lambda: div(vocabulary=v, require="C=O"), "list of SMILES strings"),
            (lambda: div(vocabulary=v, require=[]), "1 to 32 patterns"),
            (lambda: div(vocabulary=v, require=["C"] * 20, forbid=["N"] * 13), "33 patterns together"),
            (lambda: div(vocabulary=v, forbid=["C", ""]), "pattern 1 is empty at position 0"),
            (lambda: div(vocabulary=v, forbid=["C" * 33]), "at most 32"),
            (lambda: div(vocabulary=v, forbid=["C", "C?"]), "no id for"),
            (lambda: div(vocabulary=v, forbid=[7]), "SMILES string"),
            (lambda: M.screen_candidates(Inv(), fwd, cond, "cpu", N_, K_, vocabulary=v, require=["C"]), "at most 64"),
            (lambda: M.screen_candidates(Inv(), fwd, cond, "cpu", N_, K_, forbid=["C"]), "give a vocabulary"),
            (lambda: M.has_substructure(wide, ["C"], v, "cpu"), "at most 64"),
            (lambda: M.has_substructure(tok.float(), ["C"], v, "cpu"), "integer"),
            (lambda: M.has_substructure(tok, ["C"], S.CHARS, "cpu"), "SmilesVocabulary"),
            (lambda: M.has_substructure(tok, "C", v, "cpu"), "list of SMILES strings"),
            (lambda: M.has_substructure(tok, ["C"] * 33, v, "cpu"), "1 to 32 patterns"),
            (lambda: M.has_substructure(tok[:, :0], ["C"], v, "cpu"), "at least one position"),
            (lambda: M.SubstructureSet(["C"], "CNO"), "SmilesVocabulary")):
        with pytest.raises(ValueError, match=what):
            call()
    assert rec.log == []
    with pytest.raises(TypeError):                                           # screen_tokens keeps its parameter list
        M.screen_tokens(fwd, tok, cond, "cpu", N_, K_, require=["C"])
    assert list(inspect.signature(M.screen_tokens).parameters) == [
        "model_forward", "tokens", "conditioning", "device", "candidates", "keep", "known_tokens", "weights", "forward_timesteps",
        "X_norm_factor", "forward_noise", "sampler", "sigma_schedule"]
    with pytest.raises(TypeError):
        M.screen_candidates(Inv(), fwd, cond, "cpu", N_, K_, requires=["C"])
    # the op refuses what the kernel does not take
    n, rows = torch.zeros(3, dtype=torch.int32), torch.zeros(3, 8, dtype=torch.int32)
    pn = lambda P: torch.zeros(P, dtype=torch.int32)  # noqa: E731
    pr = lambda P, LP=8: torch.zeros(P, LP, dtype=torch.int32)  # noqa: E731
    sub = torch.ops.mdt.sub_match
    for call, what in ((lambda: sub(n, torch.zeros(3, 65, dtype=torch.int32), n, torch.zeros(3, 65, dtype=torch.int32), pn(2), pr(2), pn(2), pr(2), 0, 0), "1 to 64"),
                       (lambda: sub(n, rows, n, rows, pn(2), pr(2, 33), pn(2), pr(2, 33), 0, 0), "1 to 32"),
                       (lambda: sub(n, rows, n, rows, pn(0), pr(0), pn(0), pr(0), 0, 0), "0 patterns"),
                       (lambda: sub(n, rows, n, rows, pn(33), pr(33), pn(33), pr(33), 0, 0), "33 patterns"),
                       (lambda: sub(n, rows.long(), n, rows, pn(2), pr(2), pn(2), pr(2), 0, 0), "int32"),
                       (lambda: sub(n, rows, n, rows, pn(2), pr(2).long(), pn(2), pr(2), 0, 0), "int32"),
                       (lambda: sub(n[:2], rows, n, rows, pn(2), pr(2), pn(2), pr(2), 0, 0), "one value per row"),
                       (lambda: sub(n, rows, n, rows, pn(3), pr(2), pn(2), pr(2), 0, 0), "one value per row"),
                       (lambda: sub(n, rows, n, rows, pn(2), pr(2), pn(2), pr(2), 4, 0), "below P"),
                       (lambda: sub(n, rows, n, rows, pn(2), pr(2), pn(2), pr(2), 0, -1), "below P"),
                       (lambda: sub(n, rows, n, rows, pn(2), pr(2), pn(2), pr(2), 3, 1), "overlap")):
        with pytest.raises(RuntimeError, match=what):
            call()
    assert rec.log == []


def test_a_pattern_that_does_not_pass_the_check_is_named_with_its_position(rec, monkeypatch):
    v = vocabulary()
    real = torch.ops.mdt

    class Stub:
        def __getattr__(self, name):
            if name != "mol_graph":
                return getattr(real, name)

            def graph(packed, n, *tables):
                out = list(real.mol_graph(packed, n, *tables))
                out[4], out[5] = torch.tensor([0, 32, 64], dtype=torch.uint8), torch.tensor([-1, 2, 0], dtype=torch.int32)
                return tuple(out)
            return graph
    three = M.SubstructureSet(["CC", "C((", "C=C=C"], v)
    monkeypatch.setattr(G.torch, "ops", type("Ops", (), {"mdt": Stub()})())
    with pytest.raises(ValueError, match=r"pattern 1 'C\(\(' does not pass smiles_check\(\): malformed at position 2"):
        three.on("cpu")


def test_the_pattern_graphs_are_cached_per_device(rec):
    v = vocabulary()
    one = M.SubstructureSet(["C=O", "c1ccccc1", "N"], v)
    assert (len(one), one.patterns, one.vocabulary, one.width) == (3, ("C=O", "c1ccccc1", "N"), v, 8) and rec.log == []
    first = one.on("cpu")
    assert names(rec) == PATTERN_GRAPHS and rec.log[1][3:5] == (8, 3)
    assert [(tuple(t.shape), t.dtype) for t in first] == [((3,), torch.int32), ((3, 8), torch.int32)] * 2
    assert one.on("cpu") is first and one.on(torch.device("cpu")) is first and len(rec.log) == 2
    one._on.clear()                                                          # (another device: computed again)
    assert one.on("cpu") is not first and len(rec.log) == 4
    assert M.SubstructureSet("CO", v).patterns == ("CO",)


def test_public_surface_and_what_the_docstrings_promise():
    assert M.has_substructure is G.has_substructure and M.SubstructureSet is G.SubstructureSet
    p = inspect.signature(M.screen_tokens_diverse).parameters
    assert (p["require"].default, p["forbid"].default) == (None, None) and list(p)[-1] == "screen_tokens_kwargs"
    assert not {"require", "forbid"} & set(inspect.signature(M.screen_tokens).parameters)
    assert list(inspect.signature(M.has_substructure).parameters) == ["tokens", "patterns", "vocabulary", "device"]
    for doc in (M.has_substructure.__doc__, M.screen_tokens_diverse.__doc__):
        flat = " ".join(doc.split())
        for phrase in ("not SMARTS", "not RDKit's HasSubstructMatch", "no implicit hydrogens", "no aromaticity perception",
                       "no stereo", "undecided"):
            assert phrase in flat, (phrase, flat[:60])
    flat = " ".join(M.has_substructure.__doc__.split())
    for phrase in ("does not depend on how row or pattern is spelled", "which pairs come out undecided can", "4096 steps",
                   "no pre-filter", "no mapping is returned", "never together with ``match``"):
        assert phrase in flat, phrase
    assert "not SMARTS" in M.SubstructureSet.__doc__ and "128" in M.screen_tokens_diverse.__doc__
