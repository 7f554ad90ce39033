"""No GPU: the definition of the graph fingerprint and its Tanimoto similarity (include/mdt_hip.h, mdt_mol_fp ...) on its reference
(tests/molfp_ref.py) -- one fingerprint per graph whatever the spelling, the agreed pairs, nesting, rows that are no molecule -- and
the plumbing: C exports and argument checks, op schemas and shape inference, the refusals, the launch order of the screening calls
with the two similarity thresholds on a recording library, the cache of KnownSet.fingerprints and what the docstrings promise."""
import contextlib
import inspect
import os
import re

import pytest
import torch

import molfp_ref as F
import molkey_ref as K
import smiles_ref as S
from conftest import ROOT
import moleculediffusiontransformer_amd as M
from moleculediffusiontransformer_amd import generative as G, ops, runtime as rt


@pytest.fixture(scope="module")
def spelled():
    return K.random_spellings()


def similarity_is_one(a, b):
    inter, union = F.counts(a, b)
    return union > 0 and inter == union


# ---------------------------------------------------------------------------------------------------------------------
# the definition on the reference
# ---------------------------------------------------------------------------------------------------------------------
def test_every_spelling_of_a_graph_gives_one_fingerprint(spelled):
    distinct = set()
    for g, sp in spelled:
        for radius in (0, 2):
            fps = {F.string_fp(s, radius) for s in sp} | {F.fingerprint(g.descriptors(), g.bonds, radius)}
            assert len(fps) == 1 and 0 not in fps, (sp, radius)
        fp = F.string_fp(sp[0])
        assert 1 <= F.popcount(fp) <= 3 * len(g.atoms)                       # count <= (radius + 1) * natoms
        assert similarity_is_one(fp, F.string_fp(sp[-1]))
        distinct.add(fp)
    assert len(distinct) >= 0.9 * len({K.string_key(sp[0]) for _, sp in spelled})      # it does tell molecules apart


@pytest.mark.parametrize("a,b", K.EQUAL_PAIRS)
def test_equal_pairs_have_similarity_exactly_one(a, b):
    assert F.string_fp(a) == F.string_fp(b) != 0 and similarity_is_one(F.string_fp(a), F.string_fp(b))
    assert F.at_least(*F.counts(F.string_fp(a), F.string_fp(b)), F.SIM_DEN)


# (the other pairs of DIFFERENT_PAIRS differ in how equal atoms are connected, which a radius-2 neighbourhood need not see)
ATOM_OR_ORDER = [("CCO", "COC"), ("CC=O", "C=CO"), ("C[NH3+]", "CN"), ("c1ccccc1", "C1=CC=CC=C1"), ("C1CCCCC1", "CCCCCC"),
                 ("CC(C)C", "CCCC")]


@pytest.mark.parametrize("a,b", ATOM_OR_ORDER)
def test_pairs_that_differ_in_an_atom_or_a_bond_order_lie_below_one(a, b):
    assert (a, b) in K.DIFFERENT_PAIRS
    inter, union = F.counts(F.string_fp(a), F.string_fp(b))
    assert 0 <= inter < union and not F.at_least(inter, union, F.SIM_DEN)


def test_count_bound_nesting_and_the_layout_of_the_words(spelled):
    for g, sp in spelled[:120]:
        fps = [F.string_fp(sp[0], r) for r in range(4)]
        for r in range(4):
            assert F.popcount(fps[r]) <= (r + 1) * len(g.atoms)
        for r in range(3):
            assert fps[r] & fps[r + 1] == fps[r] and fps[r] != 0              # radius 0..3 give nested bit sets
    d = K.descriptor("C")
    bit = K.mix(d | 0 << 32) & 1023                                          # methane at radius 0: one atom of degree 0, one bit
    assert F.fingerprint([d], [], 0) == 1 << bit and F.words(1 << bit)[bit >> 6] == 1 << (bit & 63)
    again = K.mix(K.mix(d) ^ K.mix(0)) & 1023                                # ... and round 1 hashes the label again: no neighbours, sum 0
    assert F.fingerprint([d], [], 1) == 1 << bit | 1 << again
    assert F.from_words(F.words(F.string_fp("CCO"))) == F.string_fp("CCO")
    # the degree enters round 0, a doubled bond counts twice, and the order enters round 1
    assert F.fingerprint([d, d], [(0, 1, 1)], 0) == 1 << (K.mix(d | 1 << 32) & 1023)
    assert F.fingerprint([d, d], [(0, 1, 1)] * 2, 0) == 1 << (K.mix(d | 2 << 32) & 1023)
    assert F.fingerprint([d, d], [(0, 1, 1)], 1) != F.fingerprint([d, d], [(0, 1, 2)], 1)
    assert F.fingerprint([d, d], [(0, 1, 1)], 0) == F.fingerprint([d, d], [(0, 1, 2)], 0)


def test_rows_that_are_no_molecule():
    ethanol = F.string_fp("CCO")
    for s in [""] + [s for s, _ in S.MALFORMED_TABLE + S.OVERVALENT_TABLE]:
        assert F.string_fp(s) == 0, s
        for other in (ethanol, 0):
            assert F.counts(0, other)[0] == 0 and not F.at_least(*F.counts(0, other), 1)          # similarity 0 to everything
    d = K.descriptor("C")
    assert F.fingerprint([d] * 3, [(0, 3, 1)], 2) == 0 and F.fingerprint([d] * 9, [], 2, width=8) == 0
    assert F.nearest(0, [ethanol, 0]) == (0, 0, F.popcount(ethanol)) and F.nearest(ethanol, [0, 0])[0] == 0
    assert all(F.string_fp(s) != 0 for s in S.OK_TABLE if s)


# ---------------------------------------------------------------------------------------------------------------------
# header, library, binding
# ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_the_library_exports_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "mdt_hip.h")).read()
    lib = rt.load_library()
    for name, arity in (("mdt_mol_fp", 10), ("mdt_fp_tanimoto_rows", 6), ("mdt_fp_nearest", 9), ("mdt_screen_select_similar", 23)):
        assert re.search(r"\bint %s\s*\(" % name, hdr) and name in rt.SYMBOLS and hasattr(lib, name), name
        assert len(rt.SYMBOLS[name][1]) == arity
    assert int(re.search(r"#define MDT_ABI_VERSION (\d+)", hdr).group(1)) == rt.ABI_VERSION == 5 == lib.mdt_abi_version()
    assert int(re.search(r"#define MDT_FP_BITS (\d+)", hdr).group(1)) == rt.FP_BITS == 64 * rt.FP_WORDS == F.BITS
    assert int(re.search(r"#define MDT_FP_SIM_DEN (\d+)", hdr).group(1)) == rt.FP_SIM_DEN == G.FP_SIM_DEN == F.SIM_DEN
    assert int(re.search(r"#define MDT_FP_KNOWN_CHUNK (\d+)", hdr).group(1)) == rt.FP_KNOWN_CHUNK
    for phrase in ("not RDKit's Morgan or ECFP", "no implicit hydrogens", "Duplicate substructures are not removed",
                   "no aromaticity perception", "no stereo", "share a bit", "Equal graphs always give equal fingerprints",
                   "inter * 65536 >= sim_num * union"):
        assert phrase in hdr, phrase
    assert "k_molfp.hip" in [s for s, _ in __import__("moleculediffusiontransformer_amd.build", fromlist=["SOURCES"]).SOURCES]


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = rt.load_library()

    def fp(L=32, R_=5, radius=2, p=8, out=8):
        return lib.mdt_mol_fp(p, p, p, p, L, R_, radius, out, out, 0)

    def rows(R_=5, p=8, out=8):
        return lib.mdt_fp_tanimoto_rows(p, p, R_, out, out, 0)

    def nearest(R_=5, M_=3, p=8, out=8):
        return lib.mdt_fp_nearest(p, R_, p, M_, out, out, out, out, 0)

    def similar(L=32, N=4, G_=3, K_=2, M_=0, sim=100, p=8, fpp=8, cnt=8):
        return lib.mdt_screen_select_similar(p, p, p, p, L, N, G_, 0, 0, 0, M_, K_, 0, 1, 1, 0, fpp, cnt, sim, p, p, p, 0)
    for call, kw, what in ((fp, dict(L=0), b"L <= 64"), (fp, dict(L=65), b"L <= 64"), (fp, dict(R_=-1), b"R >= 0"),
                           (fp, dict(radius=-1), b"radius"), (fp, dict(radius=4), b"radius"), (fp, dict(p=0), b"null"),
                           (fp, dict(out=0), b"null"), (rows, dict(R_=-1), b"R >= 0"), (rows, dict(p=0), b"null"),
                           (rows, dict(out=0), b"null"), (nearest, dict(M_=0), b"M >= 1"), (nearest, dict(R_=-1), b"R >= 0"),
                           (nearest, dict(p=0), b"null"), (nearest, dict(out=0), b"null"),
                           (similar, dict(sim=0), b"sim_num"), (similar, dict(sim=65537), b"sim_num"), (similar, dict(N=0), b"N <= 1024"),
                           (similar, dict(N=1025), b"N <= 1024"), (similar, dict(K_=0), b"K <= N"), (similar, dict(K_=5), b"K <= N"),
                           (similar, dict(L=65), b"L <= 64"), (similar, dict(L=0), b"L <= 64"), (similar, dict(M_=2), b"NULL only"),
                           (similar, dict(p=0), b"null"), (similar, dict(cnt=0), b"null"), (similar, dict(fpp=0), b"null")):
        assert call(**kw) != 0, (call.__name__, kw)
        assert what in lib.mdt_last_error(), (call.__name__, kw, lib.mdt_last_error())
    # nothing to do: nothing is launched, nothing is read
    assert fp(R_=0) == 0 and fp(R_=0, p=0, out=0) == 0 and rows(R_=0) == 0 and rows(R_=0, p=0, out=0) == 0
    assert nearest(R_=0) == 0 and nearest(R_=0, p=0, out=0) == 0 and similar(G_=0) == 0 and similar(G_=0, p=0) == 0
    assert nearest(R_=0, M_=0) != 0 and similar(G_=0, sim=0) != 0            # ... but a bad argument is still one


def vocabulary():
    return M.SmilesVocabulary([None] + S.CHARS)


def test_ops_schema_and_shape_inference():
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert str(torch.ops.mdt.mol_fp.default._schema) == \
        "mdt::mol_fp(Tensor natoms, Tensor atoms, Tensor nbonds, Tensor bonds, SymInt radius) -> (Tensor, Tensor)"
    assert str(torch.ops.mdt.fp_tanimoto.default._schema) == "mdt::fp_tanimoto(Tensor a_fp, Tensor b_fp) -> (Tensor, Tensor)"
    assert str(torch.ops.mdt.fp_nearest.default._schema) == "mdt::fp_nearest(Tensor fp, Tensor known_fp) -> (Tensor, Tensor, Tensor)"
    assert str(torch.ops.mdt.screen_select_similar.default._schema) == \
        ("mdt::screen_select_similar(Tensor score, Tensor key, Tensor packed, Tensor length, SymInt candidates, SymInt keep, "
         "Tensor? known_key, Tensor? known_packed, Tensor? known_len, Tensor? known_dist, SymInt min_novelty, SymInt min_distance, "
         "Tensor? reject, Tensor? fp, Tensor? fp_count, SymInt sim_num) -> (Tensor, Tensor, Tensor)")
    with FakeTensorMode():
        n, rows = torch.empty(15, dtype=torch.int32), torch.empty(15, 40, dtype=torch.int32)
        fp, count = torch.ops.mdt.mol_fp(n, rows, n, rows, 2)
        assert (tuple(fp.shape), fp.dtype, tuple(count.shape), count.dtype) == ((15, 16), torch.int64, (15,), torch.int32)
        out = torch.ops.mdt.fp_tanimoto(fp, fp)
        assert [(tuple(t.shape), t.dtype) for t in out] == [((15,), torch.int32)] * 2
        out = torch.ops.mdt.fp_nearest(fp, torch.empty(7, 16, dtype=torch.int64))
        assert [(tuple(t.shape), t.dtype) for t in out] == [((15,), torch.int32)] * 3
        score, key = torch.empty(15), torch.empty(15, dtype=torch.int64)
        out = torch.ops.mdt.screen_select_similar(score, key, rows, n, 5, 2, None, None, None, None, 1, 1, None, fp, count, 100)
        assert [(tuple(t.shape), t.dtype) for t in out] == [((15,), torch.uint8), ((3, 2), torch.int32), ((3,), torch.int32)]
    n, rows = torch.zeros(3, dtype=torch.int32), torch.zeros(3, 4, dtype=torch.int32)       # no CPU implementation behind the ops
    fp = torch.zeros(3, 16, dtype=torch.int64)
    for call in (lambda: torch.ops.mdt.mol_fp(n, rows, n, rows, 2), lambda: torch.ops.mdt.fp_tanimoto(fp, fp),
                 lambda: torch.ops.mdt.fp_nearest(fp, fp)):
        with pytest.raises(RuntimeError, match="no CPU implementation"):
            call()


# ---------------------------------------------------------------------------------------------------------------------
# on a recording library: launch order for every combination of the keywords, refusals with nothing launched
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
HEAD = ["mdt_tokens_compact", "forward_sample", "mdt_screen_score"]


def names(rec):
    return [e[0] for e in rec.log]


def test_launch_order_for_each_combination_of_the_keywords(rec):
    tok, cond, v = torch.ones(N_ * G_, L_, dtype=torch.long), torch.zeros(G_, n_), vocabulary()
    known = M.KnownSet(torch.ones(4, L_, dtype=torch.long), L_)
    run = lambda **kw: (rec.log.clear(), M.screen_tokens_diverse(Fwd(rec), tok, cond, "cpu", N_, K_, **kw), names(rec)[3:])[2]  # noqa: E731
    # max_similarity alone: the graph and the fingerprint once, then the new selection
    assert run(vocabulary=v, max_similarity=0.5) == ["mdt_smiles_check", "mdt_mol_graph", "mdt_mol_fp", "mdt_screen_select_similar"]
    compact, _, _, check, graph, fp, select = rec.log
    assert fp[1:8] == (graph[8], graph[9], graph[10], graph[11], L_, N_ * G_, 2) and len(select) == 1 + 23
    assert select[16] == check[8] and select[17:20] == (fp[8], fp[9], 32768) and select[13:16] == (0, 1, 1)
    assert run(vocabulary=v, max_similarity=1.0, fingerprint_radius=3, min_distance=3)[-2:] == ["mdt_mol_fp", "mdt_screen_select_similar"]
    assert rec.log[-2][7] == 3 and rec.log[-1][15] == 3 and rec.log[-1][19] == 65536
    # max_known_similarity alone: the known set's fingerprints once per (vocabulary, device, radius), the search, today's selection
    for again in (False, True):
        middle = [] if again else ["mdt_mol_graph", "mdt_mol_fp"]
        assert run(vocabulary=v, known_tokens=known, max_known_similarity=0.7) == \
            ["mdt_smiles_check", "mdt_mol_graph", "mdt_mol_fp"] + middle + ["mdt_fp_nearest", "mdt_screen_select_reject"]
    nearest, select = rec.log[-2], rec.log[-1]
    assert nearest[2] == N_ * G_ and nearest[4] == len(known) and select[13] not in (0, rec.log[3][8])     # reject = the check's | bit 8
    # both, with graph identity: ONE mdt_mol_graph over the candidates feeds the key and the fingerprint
    assert run(vocabulary=v, known_tokens=known, identity="graph", max_similarity=0.4, max_known_similarity=0.7, min_novelty=2) == \
        ["mdt_smiles_check", "mdt_mol_graph", "mdt_mol_key", "mdt_mol_graph", "mdt_mol_key", "mdt_key_flags", "mdt_mol_fp",
         "mdt_fp_nearest", "mdt_edit_nearest", "mdt_screen_select_similar"]
    assert run(vocabulary=v, known_tokens=known, max_similarity=0.4, max_known_similarity=0.7, min_distance=2) == \
        ["mdt_smiles_check", "mdt_mol_graph", "mdt_mol_fp", "mdt_fp_nearest", "mdt_screen_select_similar"]
    assert run(vocabulary=v, known_tokens=known, max_known_similarity=0.7, min_distance=2)[-2:] == \
        ["mdt_fp_nearest", "mdt_screen_select_diverse_reject"]
    # with both at None the launches are those made before the keywords existed
    parent = {(): ["mdt_screen_select"], (("vocabulary", v),): ["mdt_smiles_check", "mdt_screen_select_reject"],
              (("min_distance", 2),): ["mdt_screen_select_diverse"],
              (("vocabulary", v), ("min_distance", 2)): ["mdt_smiles_check", "mdt_screen_select_diverse_reject"],
              (("known_tokens", known), ("min_novelty", 2)): ["mdt_edit_nearest", "mdt_screen_select_diverse"],
              (("vocabulary", v), ("identity", "graph")): ["mdt_smiles_check", "mdt_mol_graph", "mdt_mol_key", "mdt_key_flags",
                                                          "mdt_screen_select_reject"]}
    for kw, want in parent.items():
        logs = []
        for extra in (dict(), dict(max_similarity=None, max_known_similarity=None, fingerprint_radius=1)):
            assert run(**dict(kw), **extra) == want, kw
            logs.append([(e[0], len(e), tuple(a for a in e[1:] if isinstance(a, int) and a < 4096)) for e in rec.log])
        assert logs[0] == logs[1]
    # the public calls
    rec.log.clear()
    fp, count, status, position = M.mol_fingerprint(tok.to(torch.int16), v, "cpu")
    assert names(rec) == ["mdt_tokens_compact", "mdt_mol_graph", "mdt_mol_fp"] and rec.log[2][5:8] == (L_, N_ * G_, 2)
    assert fp.shape == (N_ * G_, 16) and all(t.dtype == torch.int64 and t.shape == (N_ * G_,) for t in (count, status, position))
    rec.log.clear()
    sim, inter, union = M.tanimoto(tok, tok, v, "cpu", radius=1)
    assert names(rec) == ["mdt_tokens_compact", "mdt_mol_graph", "mdt_mol_fp"] * 2 + ["mdt_fp_tanimoto_rows"] and rec.log[2][7] == 1
    assert sim.dtype == torch.float32 and inter.dtype == union.dtype == torch.int64 and sim.shape == inter.shape == (N_ * G_,)
    rec.log.clear()
    sim, index, inter, union = M.nearest_known_tanimoto(tok, known, v, "cpu")
    assert names(rec) == ["mdt_tokens_compact", "mdt_mol_graph", "mdt_mol_fp", "mdt_fp_nearest"]       # (the known side is cached)
    assert sim.dtype == torch.float32 and index.dtype == torch.int64 and index.shape == (N_ * G_,)


def test_screen_candidates_takes_the_thresholds(rec, monkeypatch):
    seen = {}

    class Inv:
        max_length = 32

        def sample_tokens(self, seq, device, **k):
            return torch.ones(seq.shape[0], 32, dtype=torch.long)
    monkeypatch.setattr(G, "screen_tokens", lambda *a, **k: seen.update(plain=k) or "plain")
    monkeypatch.setattr(G, "screen_tokens_diverse", lambda *a, **k: seen.update(diverse=k) or "diverse")
    cond, v = torch.zeros(2, 12), vocabulary()
    assert M.screen_candidates(Inv(), "fwd", cond, "dev", 3, 2, vocabulary=v, max_similarity=0.5, fingerprint_radius=1) == "diverse"
    assert seen["diverse"] == dict(min_distance=1, min_novelty=1, vocabulary=v, max_similarity=0.5, fingerprint_radius=1)
    assert M.screen_candidates(Inv(), "fwd", cond, "dev", 3, 2, max_similarity=None, max_known_similarity=None) == "plain"
    assert seen["plain"] == dict()                                           # as without the keywords
    assert list(inspect.signature(M.screen_candidates).parameters)[-1] == "screen_tokens_kwargs"


def test_refusals_come_before_anything_is_launched(rec):
    fwd, v = Fwd(rec), vocabulary()
    tok, cond = torch.ones(N_ * G_, L_, dtype=torch.long), torch.zeros(G_, n_)
    wide = torch.ones(N_ * G_, 65, dtype=torch.long)
    known, empty = M.KnownSet(tok[:4], L_), M.KnownSet(tok[:0], L_)
    div = lambda t=tok, **kw: M.screen_tokens_diverse(fwd, t, cond, "cpu", N_, K_, **kw)  # noqa: E731

    class Inv:
        max_length = 65

        def sample_tokens(self, *a, **k):
            raise AssertionError("sampled")
    for call, what in (
            (lambda: div(max_similarity=0.5), "give a vocabulary"),
            (lambda: div(max_known_similarity=0.5, known_tokens=known), "give a vocabulary"),
            (lambda: div(wide, vocabulary=v, max_similarity=0.5), "at most 64"),
            (lambda: div(vocabulary=v, max_similarity=0.0), r"\(0, 1\]"),
            (lambda: div(vocabulary=v, max_similarity=1.5), r"\(0, 1\]"),
            (lambda: div(vocabulary=v, max_similarity=True), r"\(0, 1\]"),
            (lambda: div(vocabulary=v, max_similarity="0.5"), r"\(0, 1\]"),
            (lambda: div(vocabulary=v, max_similarity=1e-9), "sim_num = 0"),
            (lambda: div(vocabulary=v, max_known_similarity=0.5), "non-empty"),
            (lambda: div(vocabulary=v, max_known_similarity=0.5, known_tokens=empty), "non-empty"),
            (lambda: div(vocabulary=v, max_similarity=0.5, fingerprint_radius=4), "radius"),
            (lambda: div(vocabulary=v, max_similarity=0.5, fingerprint_radius=1.0), "radius"),
            (lambda: M.screen_candidates(Inv(), fwd, cond, "cpu", N_, K_, vocabulary=v, max_similarity=0.5), "at most 64"),
            (lambda: M.screen_candidates(Inv(), fwd, cond, "cpu", N_, K_, max_known_similarity=0.5), "give a vocabulary"),
            (lambda: M.mol_fingerprint(wide, v, "cpu"), "at most 64"),
            (lambda: M.mol_fingerprint(tok, v, "cpu", radius=-1), "radius"),
            (lambda: M.mol_fingerprint(tok.float(), v, "cpu"), "integer"),
            (lambda: M.mol_fingerprint(tok, S.CHARS, "cpu"), "SmilesVocabulary"),
            (lambda: M.tanimoto(tok, tok[:3], v, "cpu"), "same shape"),
            (lambda: M.tanimoto(wide, wide, v, "cpu"), "at most 64"),
            (lambda: M.nearest_known_tanimoto(tok, empty, v, "cpu"), "empty"),
            (lambda: M.nearest_known_tanimoto(wide, wide, v, "cpu"), "at most 64"),
            (lambda: M.nearest_known_tanimoto(tok, M.KnownSet(tok, 20), v, "cpu"), "built for rows of 20"),
            (lambda: M.nearest_known_tanimoto(tok, known, "CNO", "cpu"), "SmilesVocabulary"),
            (lambda: M.KnownSet(wide, 65).fingerprints(v, "cpu"), "at most 64"),
            (lambda: known.fingerprints(v, "cpu", radius=7), "radius")):
        with pytest.raises(ValueError, match=what):
            call()
    assert rec.log == []
    with pytest.raises(TypeError):                                           # screen_tokens keeps its parameter list
        M.screen_tokens(fwd, tok, cond, "cpu", N_, K_, max_similarity=0.5)
    with pytest.raises(TypeError):
        M.screen_candidates(Inv(), fwd, cond, "cpu", N_, K_, max_simlarity=0.5)
    # the ops refuse what the kernels do not take
    rec.log.clear()
    n, rows, fp = torch.zeros(3, dtype=torch.int32), torch.zeros(3, 8, dtype=torch.int32), torch.zeros(3, 16, dtype=torch.int64)
    score, key = torch.zeros(3), torch.zeros(3, dtype=torch.int64)
    for call, what in ((lambda: torch.ops.mdt.mol_fp(n, torch.zeros(3, 65, dtype=torch.int32), n, torch.zeros(3, 65, dtype=torch.int32), 2), "1 to 64"),
                       (lambda: torch.ops.mdt.mol_fp(n, rows, n, rows, 4), "radius"),
                       (lambda: torch.ops.mdt.mol_fp(n, rows.long(), n, rows, 2), "int32"),
                       (lambda: torch.ops.mdt.mol_fp(n[:2], rows, n, rows, 2), "one value per row"),
                       (lambda: torch.ops.mdt.fp_tanimoto(fp, fp[:2]), "same shape"),
                       (lambda: torch.ops.mdt.fp_tanimoto(fp[:, :8], fp[:, :8]), "int64"),
                       (lambda: torch.ops.mdt.fp_nearest(fp, fp[:0]), "empty"),
                       (lambda: torch.ops.mdt.fp_nearest(fp.int(), fp), "int64"),
                       (lambda: torch.ops.mdt.screen_select_similar(score, key, rows, n, 3, 1, None, None, None, None, 1, 1, None, fp, None, 5),
                        "come together"),
                       (lambda: torch.ops.mdt.screen_select_similar(score, key, rows, n, 3, 1, None, None, None, None, 1, 1, None, fp, n, 0),
                        "sim_num"),
                       (lambda: torch.ops.mdt.screen_select_similar(score, key, rows, n, 3, 1, None, None, None, None, 1, 1, None, fp[:2], n, 5),
                        "per row")):
        with pytest.raises(RuntimeError, match=what):
            call()
    assert rec.log == []


def test_known_fingerprints_are_cached_per_vocabulary_device_and_radius(rec):
    known = M.KnownSet(torch.arange(1, 9).reshape(8, 1).repeat(1, 2), 4)
    v, w = vocabulary(), vocabulary()
    first = known.fingerprints(v, "cpu")
    assert names(rec) == ["mdt_mol_graph", "mdt_mol_fp"] and rec.log[1][6:8] == (len(known), 2)
    assert first[0].shape == (len(known), 16) and first[0].dtype == torch.int64 and first[1].dtype == torch.int32       # ALL rows, in order
    assert known.fingerprints(v, "cpu") is first and known.fingerprints(v, "cpu", radius=2) is first and len(rec.log) == 2
    assert known.fingerprints(v, "cpu", radius=1) is not first and rec.log[-1][7] == 1 and len(rec.log) == 4
    assert known.fingerprints(w, "cpu") is not first and len(rec.log) == 6
    assert known.fingerprints(w, "cpu") is known.fingerprints(w, "cpu") and len(rec.log) == 6


def test_public_surface_and_what_the_docstrings_promise():
    assert M.mol_fingerprint is G.mol_fingerprint and M.tanimoto is G.tanimoto and M.nearest_known_tanimoto is G.nearest_known_tanimoto
    p = inspect.signature(M.screen_tokens_diverse).parameters
    assert (p["max_similarity"].default, p["max_known_similarity"].default, p["fingerprint_radius"].default) == (None, None, 2)
    assert not {"max_similarity", "max_known_similarity"} & set(inspect.signature(M.screen_tokens).parameters)
    for fn in (M.mol_fingerprint, M.tanimoto, M.nearest_known_tanimoto):
        assert inspect.signature(fn).parameters["radius"].default == 2
    for doc in (M.mol_fingerprint.__doc__, M.tanimoto.__doc__, M.nearest_known_tanimoto.__doc__, M.screen_tokens_diverse.__doc__):
        flat = " ".join(doc.split())
        for phrase in ("not RDKit's Morgan or ECFP", "no implicit hydrogens", "no aromaticity perception", "no stereo"):
            assert phrase in flat, (phrase, flat[:60])
    flat = " ".join(M.mol_fingerprint.__doc__.split())
    for phrase in ("duplicate substructures are not removed", "folding to 1024 bits can make unequal environments share a bit",
                   "Equal graphs always give equal fingerprints"):
        assert phrase in flat, phrase
    assert "in that order" in M.KnownSet.fingerprints.__doc__ and "all-zero" in M.KnownSet.fingerprints.__doc__
