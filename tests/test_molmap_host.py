"""No GPU: the definition of the substructure enumeration (include/mdt_hip.h, mdt_sub_map) on its reference (tests/molmap_ref.py)
-- every output word against a brute force over all injective maps, agreement with the first-success search of molsub_ref on
every pair, counts that do not depend on the spelling, the step cap and the flag arithmetic -- the shared C++ search on the host
under AddressSanitizer and UBSan (tools/molmap_host_check.cpp), and the plumbing: C export and argument checks, op schema and
shape inference, the refusals, the launch order of the calls with and without ``counts=`` on a recording library, and what the
docstrings promise."""
import contextlib
import inspect
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

import molkey_ref as K
import molmap_ref as A
import molsub_ref as B
import smiles_ref as S
from conftest import ROOT
import moleculediffusiontransformer_amd as M
from moleculediffusiontransformer_amd import generative as G, ops, runtime as rt
from moleculediffusiontransformer_amd import SubstructureCounts, substructure_keep, substructure_map     # what this file is about

CAP_PATTERN, CAP_MATCH, CAP_UNDECIDED = "C.C.C.C.C.C.CN", "C" * 61 + "CN", "C" * 62 + ".N"
# at most 7 atoms a target, at most 4 a pattern: at most 7 * 6 * 5 * 4 = 840 injective maps a pair
SMALL_TARGETS = ["c1ccccc1", "C(F)(F)F", "FC(F)(F)C", "OCO", "CCC", "C1CC1", "C1CC1C", "CC(=O)O", "C.C", "C.CO", "N#CC#N", "C",
                 "CC(C)(C)C", "C1CCC1", "[NH3+]CC[O-]", "c1ccncc1", "C=CC=C", "OC(=O)C(=O)O", "C1CC1.C", "[Na+].[Cl-]", "C(C1)1", "OCCOCCO",
                 "C12CC1C2", "FC(F)(F)C(F)F"]
SMALL_PATTERNS = ["cccc", "C(F)(F)F", "CO", "CC", "C1CC1", "C.C", "*", "C", "C=O", "*.*", "C*C", "O", "ccc", "c:c", "C#N", "[O-]",
                  "C(C)(C)C", "C1CCC1", "**", "OC=O", "C.O.C", "cn", "C(C1)1", "*1**1"]


def popcount(w):
    return bin(w).count("1")


def pair_words(pattern, target):
    (pa, pb), (ta, tb) = B.graph_of(pattern), B.graph_of(target)
    return (len(ta), ta, len(tb), tb, len(pa), pa, len(pb), pb)


@pytest.fixture(scope="module")
def spelled():
    return K.random_spellings()


# ---------------------------------------------------------------------------------------------------------------------
# the definition on the reference
# ---------------------------------------------------------------------------------------------------------------------
def test_every_output_word_against_all_injective_maps():
    """found is the set of f(0), embeddings the number of valid maps, cover the union of the images, map the lexicographic minimum:
    the checker (molmap_ref.brute_force) tests each of the n! / (n - m)! injective maps with the atom and bond rules alone."""
    pairs = matching = 0
    for t in SMALL_TARGETS:
        assert 1 <= len(B.graph_of(t)[0]) <= 7, t
        for p in SMALL_PATTERNS:
            args = pair_words(p, t)
            m = args[4]
            assert 1 <= m <= 4, p
            maps = A.brute_force(*args)
            got = A.map_arrays(*args)
            assert got["capped"] == 0, (p, t)
            assert got["found"] == sum(1 << r for r in {f[0] for f in maps}), (p, t)
            assert got["embeddings"] == len(maps), (p, t)
            assert got["cover"] == sum(1 << a for a in {a for f in maps for a in f}), (p, t)
            assert got["map"] == ([1 + a for a in min(maps)] + [0] * (B.MAX_WIDTH - m) if maps else [0] * B.MAX_WIDTH), (p, t)
            pairs += 1
            matching += bool(maps)
    assert pairs >= 200 and 0.2 * pairs < matching < 0.8 * pairs
    by = lambda p, t: A.string_map(p, t)  # noqa: E731
    assert by("cccc", "c1ccccc1")["embeddings"] == 12 and by("cccc", "c1ccccc1")["found"] == 0b111111
    cf3 = by("C(F)(F)F", "FC(F)(F)C")                                        # anchors, not atom sets: one CF3 carbon, six maps
    assert (cf3["found"], cf3["embeddings"], cf3["cover"], cf3["map"][:4]) == (0b00010, 6, 0b01111, [2, 1, 3, 4])
    assert by("CO", "OCO")["found"] == 0b010 and by("CO", "OCO")["embeddings"] == 2 and by("CO", "OCO")["cover"] == 0b111
    assert by("CC", "CCC")["found"] == 0b111 and by("CC", "CCC")["embeddings"] == 4       # every carbon with a carbon neighbour
    assert by("C1CC1", "C1CC1")["embeddings"] == 6 and by("C.C", "CCC")["embeddings"] == 6 and by("*", "OCO")["map"][0] == 1


def test_agreement_with_the_first_success_search_on_every_pair():
    """found != 0 is molsub_ref's MATCH, found == 0 and capped != 0 its UNDECIDED; a root's steps up to its first success are that
    search's steps (a root that saw nothing made exactly its steps)."""
    targets = SMALL_TARGETS + ["C" * 64, "c1ccccc1" * 8, "*" * 64, "", "C(", CAP_UNDECIDED, CAP_MATCH, "N" + "C" * 63, "C" * 40 + "N"]
    patterns = SMALL_PATTERNS + ["C" * 32, "*.*.*.*", CAP_PATTERN, "NC", "c1ccccc1c1ccccc1"]
    pairs = capped = 0
    for t in targets:
        for p in patterns:
            args = pair_words(p, t)
            old, old_roots = B.match_arrays(*args)
            got = A.map_arrays(*args)
            assert (got["found"] != 0) == (old == B.MATCH), (p, t)
            assert (got["found"] == 0 and got["capped"] != 0) == (old == B.UNDECIDED), (p, t)
            assert [r for r, _, _, _ in got["roots"]] == [r for r, _, _ in old_roots]
            for (r, seen, cut, steps), (_, verdict, old_steps) in zip(got["roots"], old_roots):
                assert (seen > 0) == (verdict == B.MATCH) and (cut and not seen) == (verdict == B.UNDECIDED) and steps >= old_steps
                assert seen or steps == old_steps
            pairs += 1
            capped += got["capped"] != 0
    assert pairs > 900 and capped > 0
    high = A.string_map("NC", "C" * 40 + "N")                                # the only root is atom 40
    assert high["found"] == 1 << 40 and high["cover"] == 3 << 39 and high["map"][:2] == [41, 40] and high["embeddings"] == 1


def test_counts_do_not_depend_on_the_spelling_and_no_pair_of_the_pools_is_capped(spelled):
    """The condition that lets the GPU tests take their rows from these pools: over random_spellings() x the 27 patterns count,
    embeddings and popcount(cover) are equal for all spellings of a graph, and no root runs into the cap."""
    worst = capped = pairs = 0
    for g, sp in spelled:
        for p in B.PATTERNS:
            results = [A.string_map(p, t) for t in sp]
            assert len({(popcount(w["found"]), w["embeddings"], popcount(w["cover"])) for w in results}) == 1, (p, sp)
            capped += sum(w["capped"] != 0 for w in results)
            worst = max([worst] + [steps for w in results for _, _, _, steps in w["roots"]])
            pairs += len(results)
    print("most steps of an enumerated root: %d over %d pairs; %d with a capped root" % (worst, pairs, capped))
    assert capped == 0 and worst < B.MAX_STEPS and pairs == 54000


def test_the_cap_and_the_flag_arithmetic():
    # the existing reference: in 61 carbons, CN the roots 0..60 succeed after 62 steps, root 61 (whose seven C are then short of one:
    # the last carbon must stay free for CN) is capped without success
    _, roots = B.match_arrays(*pair_words(CAP_PATTERN, CAP_MATCH))
    assert [(r, v) for r, v, _ in roots[:61]] == [(r, B.MATCH) for r in range(61)] and all(s == 62 for _, _, s in roots[:61])
    assert roots[61][1:] == (B.UNDECIDED, 4096) and len(roots) == 62
    # under enumeration the others go on to the cap too
    got = A.map_arrays(*pair_words(CAP_PATTERN, CAP_MATCH))
    assert got["found"] == (1 << 61) - 1 and got["capped"] == (1 << 62) - 1 and B.MAX_STEPS == 4096
    assert all(cut and steps == 4096 for _, _, cut, steps in got["roots"]) and got["embeddings"] == sum(s for _, s, _, _ in got["roots"])
    assert got["map"][:8] == [1, 2, 3, 4, 5, 6, 62, 63] and popcount(got["cover"]) == 63
    c, u = popcount(got["found"]), popcount(got["capped"] & ~got["found"])
    assert (c, u) == (61, 1)
    for lo, hi, want in ((0, 255, 0), (61, 62, 0), (62, 255, 128), (0, 61, 128), (0, 62, 0), (0, 64, 0), (61, 61, 128)):
        assert A.count_flag([got["found"]], [got["capped"]], [lo], [hi]) == want, (lo, hi)
    # 62 carbons and a lone N: all capped, none found
    none = A.map_arrays(*pair_words(CAP_PATTERN, CAP_UNDECIDED))
    assert none["found"] == 0 and none["capped"] == (1 << 62) - 1 and none["embeddings"] == 0 and none["cover"] == 0 and not any(none["map"])
    c, u = popcount(none["found"]), popcount(none["capped"] & ~none["found"])
    assert (c, u) == (0, 62)
    for lo, hi, want in ((0, 255, 0), (0, 64, 0), (0, 62, 0), (0, 61, 128), (1, 255, 128), (0, 0, 128)):
        assert A.count_flag([none["found"]], [none["capped"]], [lo], [hi]) == want, (lo, hi)
    # one pattern outside its bounds is enough, and a row that is no molecule has count 0
    assert A.count_flag([1, 3], [0, 0], [0, 0], [1, 1]) == 128 and A.count_flag([1, 3], [0, 0], [1, 2], [1, 2]) == 0
    assert A.count_flag([0], [0], [0], [0]) == 0 and A.count_flag([0], [0], [1], [255]) == 128
    assert A.string_map("C", "C(") == dict(found=0, capped=0, embeddings=0, cover=0, map=[0] * 32, roots=[])


# ---------------------------------------------------------------------------------------------------------------------
# the shared C++ search on the host, under AddressSanitizer and UBSan
# ---------------------------------------------------------------------------------------------------------------------
def test_the_host_program_agrees_with_the_reference_under_the_sanitizers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import molmap_host_rows
    rows, exe = str(tmp_path / "rows.txt"), str(tmp_path / "molmap_host_check")
    pairs = molmap_host_rows.main(rows, graphs=40)
    subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "molmap_host_check.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe, rows], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    assert f" {pairs} pairs" in r.stdout and r.stdout.rstrip().endswith(" 0 wrong") and "(0 with a capped root)" not in r.stdout


# ---------------------------------------------------------------------------------------------------------------------
# header, library, binding
# ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_the_library_exports_the_new_symbol():
    hdr = open(os.path.join(ROOT, "include", "mdt_hip.h")).read()
    lib = rt.load_library()
    assert re.search(r"\bint mdt_sub_map\s*\(", hdr) and "mdt_sub_map" in rt.SYMBOLS and hasattr(lib, "mdt_sub_map")
    assert len(rt.SYMBOLS["mdt_sub_map"][1]) == 21
    assert int(re.search(r"#define MDT_ABI_VERSION (\d+)", hdr).group(1)) == rt.ABI_VERSION == 5 == lib.mdt_abi_version()
    flat = " ".join(hdr.replace(" * ", " ").split())
    for phrase in ("ANCHORS, not atom sets", "FIRST map of the LOWEST found root", "lexicographically smallest", "No root stops for another",
                   "exact when capped == 0", "count_lo[q] <= c and c + u <= count_hi[q]", "64 or more is no upper bound",
                   "distinctive atom first", "no mapping is", "atom and bond indices preserved"):
        assert phrase in flat, phrase
    src = open(os.path.join(ROOT, "moleculediffusiontransformer_amd", "csrc", "k_molsub.hip")).read()
    assert "sub_root_enumerate(" in src and "k_sub_map" in src                # the kernel runs the enumeration the host check runs
    shared = open(os.path.join(ROOT, "moleculediffusiontransformer_amd", "csrc", "mdt_molsub.h")).read()
    assert "sub_root_enumerate(" in shared and "sub_map_pair(" in shared and "sub_root_search(" in shared


def test_entry_point_refuses_bad_arguments_before_any_launch():
    lib = rt.load_library()

    def sub(L=32, R_=5, LP=8, P=3, p=8, pp=8, lo=8, hi=8, out=8, flags=8):
        return lib.mdt_sub_map(p, p, p, p, L, R_, pp, pp, pp, pp, LP, P, lo, hi, out, out, out, out, out, flags, 0)
    for kw, what in ((dict(L=0), b"L <= 64"), (dict(L=65), b"L <= 64"), (dict(R_=-1), b"R >= 0"), (dict(LP=0), b"LP <= 32"),
                     (dict(LP=33), b"LP <= 32"), (dict(P=0), b"P <= 32"), (dict(P=33), b"P <= 32"), (dict(lo=0), b"both NULL or both given"),
                     (dict(hi=0), b"both NULL or both given"), (dict(lo=0, hi=0), b"flags needs"), (dict(p=0), b"null"),
                     (dict(pp=0), b"null"), (dict(out=0), b"null")):
        assert sub(**kw) == 2, kw
        assert what in lib.mdt_last_error(), (kw, lib.mdt_last_error())
    assert sub(R_=0) == 0 and sub(R_=0, p=0, pp=0, out=0, lo=0, hi=0, flags=0) == 0      # nothing to do: nothing launched or read
    assert sub(R_=0, P=0) != 0 and sub(R_=0, lo=0) != 0 and sub(R_=0, lo=0, hi=0) != 0    # ... but a bad argument is still one


def vocabulary():
    return M.SmilesVocabulary([None] + S.CHARS)


def test_op_schema_and_shape_inference():
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert str(torch.ops.mdt.sub_map.default._schema) == \
        ("mdt::sub_map(Tensor natoms, Tensor atoms, Tensor nbonds, Tensor bonds, Tensor p_natoms, Tensor p_atoms, Tensor p_nbonds, "
         "Tensor p_bonds, Tensor? count_lo, Tensor? count_hi) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)")
    with FakeTensorMode():
        n, rows = torch.empty(15, dtype=torch.int32), torch.empty(15, 40, dtype=torch.int32)
        pn, prows = torch.empty(3, dtype=torch.int32), torch.empty(3, 9, dtype=torch.int32)
        for bounds in ((None, None), (torch.empty(3, dtype=torch.uint8),) * 2):
            out = torch.ops.mdt.sub_map(n, rows, n, rows, pn, prows, pn, prows, *bounds)
            assert [(tuple(t.shape), t.dtype) for t in out] == [((15, 3), torch.int64), ((15, 3), torch.int64), ((15, 3), torch.int32),
                                                                ((15, 3), torch.int64), ((15, 3, 9), torch.uint8), ((15,), torch.uint8)]
    n, rows = torch.zeros(3, dtype=torch.int32), torch.zeros(3, 4, dtype=torch.int32)       # no CPU implementation behind the op
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        torch.ops.mdt.sub_map(n, rows, n, rows, n, rows, n, rows, None, None)


# ---------------------------------------------------------------------------------------------------------------------
# on a recording library: launch order, refusals with nothing launched
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
NORMAL_FORM = ["mdt_mol_hydrogens", "mdt_mol_rings", "mdt_mol_normalize"]


def names(rec):
    return [e[0] for e in rec.log]


def test_launch_order_of_the_screening_call_with_and_without_counts(rec):
    tok, cond, v = torch.ones(N_ * G_, L_, dtype=torch.long), torch.zeros(G_, n_), vocabulary()
    need = M.SubstructureSet(["C=O", "N"], v)
    few = M.SubstructureCounts(["[N+](=O)[O-]", "n", "F"], v, at_least=[None, 2, 0], at_most=[1, None, 3])
    assert (few.at_least, few.at_most, len(few), few.set.patterns) == ((0, 2, 0), (1, 255, 3), 3, ("[N+](=O)[O-]", "n", "F"))
    run = lambda **kw: (rec.log.clear(), M.screen_tokens_diverse(Fwd(rec), tok, cond, "cpu", N_, K_, **kw), names(rec)[3:])[2]  # noqa: E731
    # counts alone: the candidates' graph once, the patterns' graphs the first time only, one enumeration, today's selection
    for again in (False, True):
        assert run(vocabulary=v, counts=few) == ["mdt_smiles_check", "mdt_mol_graph"] + ([] if again else PATTERN_GRAPHS) + \
            ["mdt_sub_map", "mdt_screen_select_reject"]
    check, graph, sub, select = rec.log[3:]
    assert sub[1:7] == (graph[8], graph[9], graph[10], graph[11], L_, N_ * G_) and sub[11:13] == (12, 3) and len(sub) == 1 + 21
    assert sub[7:11] == tuple(t.data_ptr() for t in few.set.on("cpu")) and sub[13:15] == tuple(t.data_ptr() for t in few.on("cpu"))
    assert few.on("cpu")[0].tolist() == [0, 2, 0] and few.on("cpu")[1].tolist() == [1, 255, 3] and few.on("cpu")[0].dtype == torch.uint8
    assert all(sub[15:21]) and select[13] not in (0, check[8])               # every output, the flags included; reject = status | flags
    # with require: the match first, then the enumeration, on one graph
    need.on("cpu")
    assert run(vocabulary=v, require=need, counts=few) == \
        ["mdt_smiles_check", "mdt_mol_graph", "mdt_sub_match", "mdt_sub_map", "mdt_screen_select_reject"]
    assert rec.log[5][1:5] == rec.log[6][1:5] == rec.log[4][8:12]
    # with normalize: counts is a consumer, and the enumeration reads the normal form
    assert run(vocabulary=v, counts=few, normalize=True) == ["mdt_smiles_check", "mdt_mol_graph"] + NORMAL_FORM + \
        ["mdt_sub_map", "mdt_screen_select_reject"]
    normal, sub = rec.log[7], rec.log[8]
    assert (sub[2], sub[4]) == (normal[11], normal[12]) and (sub[1], sub[3]) == (normal[1], normal[3])
    assert run(vocabulary=v, identity="graph", counts=few, min_distance=2) == \
        ["mdt_smiles_check", "mdt_mol_graph", "mdt_mol_key", "mdt_key_flags", "mdt_sub_map", "mdt_screen_select_diverse_reject"]
    # without it the launches are those made before the keyword existed
    for kw, want in {(): ["mdt_screen_select"], (("vocabulary", v),): ["mdt_smiles_check", "mdt_screen_select_reject"],
                     (("vocabulary", v), ("require", need)): ["mdt_smiles_check", "mdt_mol_graph", "mdt_sub_match",
                                                              "mdt_screen_select_reject"]}.items():
        logs = []
        for extra in (dict(), dict(counts=None)):
            assert run(**dict(kw), **extra) == want, kw
            logs.append([(e[0], len(e), tuple(a for a in e[1:] if isinstance(a, int) and a < 4096)) for e in rec.log])
        assert logs[0] == logs[1]


def test_launch_order_of_the_public_calls(rec):
    tok, v = torch.ones(N_ * G_, L_, dtype=torch.long), vocabulary()
    bad = M.SubstructureSet(["C#N", "OO", "c1ccccc1"], v)
    out = M.substructure_map(tok.to(torch.int16), bad, v, "cpu")
    assert names(rec) == ["mdt_tokens_compact", "mdt_mol_graph"] + PATTERN_GRAPHS + ["mdt_sub_map"]
    sub = rec.log[-1]
    assert sub[5:7] == (L_, N_ * G_) and sub[11:15] == (8, 3, 0, 0) and sub[20] == 0 and all(sub[15:20])    # no bounds, no flags
    assert out._fields == ("atom_map", "count", "found", "cover", "embeddings", "undecided", "status", "position")
    assert [(tuple(t.shape), t.dtype) for t in out] == [
        ((15, 3, 8), torch.int64), ((15, 3), torch.int64), ((15, 3, L_), torch.bool), ((15, 3, L_), torch.bool), ((15, 3), torch.int64),
        ((15, 3), torch.bool), ((15,), torch.int64), ((15,), torch.int64)]
    rec.log.clear()
    M.substructure_map(tok, bad, v, "cpu", normalize=True)
    assert names(rec) == ["mdt_tokens_compact", "mdt_mol_graph"] + NORMAL_FORM + ["mdt_sub_map"]
    assert (rec.log[-1][2], rec.log[-1][4]) == (rec.log[-2][11], rec.log[-2][12])
    # substructure_keep(): the mask is torch on the ops' outputs; with normalize the match reads the normal form and the writer
    # the graph as written
    rec.log.clear()
    out = M.substructure_keep(tok, bad, v, "cpu", occurrences="first", width=20)
    assert names(rec) == ["mdt_tokens_compact", "mdt_mol_graph", "mdt_sub_map", "mdt_mol_rank", "mdt_mol_write"]
    assert [(tuple(t.shape), t.dtype) for t in out] == [((15, 20), torch.int64), ((15, 20), torch.bool), ((15, 3), torch.bool),
                                                        ((15,), torch.bool), ((15,), torch.int64), ((15,), torch.int64), ((15,), torch.int64)]
    rec.log.clear()
    M.substructure_keep(tok, bad, v, "cpu", normalize=True, canonical=True)
    assert names(rec) == ["mdt_tokens_compact", "mdt_mol_graph"] + NORMAL_FORM + ["mdt_sub_map", "mdt_mol_rank", "mdt_mol_canon", "mdt_mol_write"]
    graph, normal, sub, write = rec.log[1], rec.log[4], rec.log[5], rec.log[8]
    assert (sub[2], sub[4]) == (normal[11], normal[12]) and write[1:5] == graph[8:12] and sub[2] != graph[9]


def test_screen_candidates_forwards_counts_only_when_given(rec, monkeypatch):
    seen = {}

    class Inv:
        max_length = 32

        def sample_tokens(self, seq, device, **k):
            return torch.ones(seq.shape[0], 32, dtype=torch.long)
    monkeypatch.setattr(G, "screen_tokens", lambda *a, **k: seen.update(plain=k) or "plain")
    monkeypatch.setattr(G, "screen_tokens_diverse", lambda *a, **k: seen.update(diverse=k) or "diverse")
    cond, v = torch.zeros(2, 12), vocabulary()
    few = M.SubstructureCounts(["F"], v, at_most=[3])
    assert M.screen_candidates(Inv(), "fwd", cond, "dev", 3, 2, vocabulary=v, counts=few) == "diverse"
    assert seen["diverse"] == dict(min_distance=1, min_novelty=1, vocabulary=v, counts=few)
    assert M.screen_candidates(Inv(), "fwd", cond, "dev", 3, 2, vocabulary=v, counts=few, normalize=True) == "diverse"
    assert seen["diverse"] == dict(min_distance=1, min_novelty=1, vocabulary=v, counts=few, normalize=True)
    assert M.screen_candidates(Inv(), "fwd", cond, "dev", 3, 2, vocabulary=v, counts=None) == "diverse"
    assert seen["diverse"] == dict(min_distance=1, min_novelty=1, vocabulary=v)
    assert M.screen_candidates(Inv(), "fwd", cond, "dev", 3, 2, counts=None) == "plain" and seen["plain"] == dict()
    for f in (M.screen_candidates, M.screen_tokens_diverse):
        assert list(inspect.signature(f).parameters)[-1] == "screen_tokens_kwargs"
    p = list(inspect.signature(M.screen_tokens_diverse).parameters)
    assert p[-3:] == ["counts", "normalize", "screen_tokens_kwargs"] and inspect.signature(M.screen_tokens_diverse).parameters["counts"].default is None
    assert "counts" not in inspect.signature(M.screen_tokens).parameters
    assert rec.log == []


def test_refusals_come_before_anything_is_launched(rec):
    fwd, v = Fwd(rec), vocabulary()
    tok, cond = torch.ones(N_ * G_, L_, dtype=torch.long), torch.zeros(G_, n_)
    wide = torch.ones(N_ * G_, 65, dtype=torch.long)
    few = M.SubstructureCounts(["F"], v, at_most=[3])
    div = lambda t=tok, **kw: M.screen_tokens_diverse(fwd, t, cond, "cpu", N_, K_, **kw)  # noqa: E731

    class Inv:
        max_length = 65

        def sample_tokens(self, *a, **k):
            raise AssertionError("sampled")
    for call, what in (
            (lambda: div(counts=few), "give a vocabulary"),
            (lambda: div(wide, vocabulary=v, counts=few), "at most 64"),
            (lambda: div(vocabulary=v, counts=["F"]), "SubstructureCounts"),
            (lambda: div(vocabulary=v, normalize=True), "normalize"),
            (lambda: M.screen_candidates(Inv(), fwd, cond, "cpu", N_, K_, vocabulary=v, counts=few), "at most 64"),
            (lambda: M.screen_candidates(Inv(), fwd, cond, "cpu", N_, K_, counts=few), "give a vocabulary"),
            (lambda: M.SubstructureCounts(["F", "N"], v, at_most=[3]), "one bound per pattern"),
            (lambda: M.SubstructureCounts(["F"], v, at_least=2), "one bound per pattern"),
            (lambda: M.SubstructureCounts(["F"], v, at_least=[-1]), "int >= 0"),
            (lambda: M.SubstructureCounts(["F"], v, at_most=[1.5]), "int >= 0"),
            (lambda: M.SubstructureCounts(["F"], v, at_most=[True]), "int >= 0"),
            (lambda: M.SubstructureCounts(["F"], v, at_least=[3], at_most=[2]), "at least 3 and at most 2"),
            (lambda: M.SubstructureCounts(["F"], v, at_least=[65]), "at least 65"),
            (lambda: M.SubstructureCounts(["F", ""], v), "pattern 1 is empty"),
            (lambda: M.SubstructureCounts(["F"], "CNO"), "SmilesVocabulary"),
            (lambda: M.substructure_map(wide, ["C"], v, "cpu"), "at most 64"),
            (lambda: M.substructure_map(tok.float(), ["C"], v, "cpu"), "integer"),
            (lambda: M.substructure_map(tok, ["C"], S.CHARS, "cpu"), "SmilesVocabulary"),
            (lambda: M.substructure_map(tok, "C", v, "cpu"), "list of SMILES strings"),
            (lambda: M.substructure_map(tok, ["C"] * 33, v, "cpu"), "1 to 32 patterns"),
            (lambda: M.substructure_map(tok[:, :0], ["C"], v, "cpu"), "at least one position"),
            (lambda: M.substructure_map(tok, ["C"], v, "cpu", normalize=1), "normalize must be"),
            (lambda: M.substructure_keep(wide, ["C"], v, "cpu"), "at most 64"),
            (lambda: M.substructure_keep(tok, ["C"], v, "cpu", occurrences="any"), "occurrences"),
            (lambda: M.substructure_keep(tok, ["C"], v, "cpu", width=129), "width"),
            (lambda: M.substructure_keep(tok, ["C" * 33], v, "cpu"), "at most 32"),
            (lambda: M.substructure_keep(tok, ["C"], v, "cpu", canonical=1), "canonical")):
        with pytest.raises(ValueError, match=what):
            call()
    assert rec.log == []
    assert M.SubstructureCounts(["F"], v, at_most=[1000]).at_most == (255,) and M.SubstructureCounts(need := M.SubstructureSet(["F"], v), v).set is need
    with pytest.raises(TypeError):                                           # screen_tokens keeps its parameter list
        M.screen_tokens(fwd, tok, cond, "cpu", N_, K_, counts=few)
    with pytest.raises(TypeError):
        M.screen_candidates(Inv(), fwd, cond, "cpu", N_, K_, count=few)
    # the op refuses what the kernel does not take
    n, rows = torch.zeros(3, dtype=torch.int32), torch.zeros(3, 8, dtype=torch.int32)
    pn = lambda P: torch.zeros(P, dtype=torch.int32)  # noqa: E731
    pr = lambda P, LP=8: torch.zeros(P, LP, dtype=torch.int32)  # noqa: E731
    u8 = lambda P: torch.zeros(P, dtype=torch.uint8)  # noqa: E731
    sub = torch.ops.mdt.sub_map
    for call, what in ((lambda: sub(n, torch.zeros(3, 65, dtype=torch.int32), n, torch.zeros(3, 65, dtype=torch.int32), pn(2), pr(2), pn(2), pr(2), None, None), "1 to 64"),
                       (lambda: sub(n, rows, n, rows, pn(2), pr(2, 33), pn(2), pr(2, 33), None, None), "1 to 32"),
                       (lambda: sub(n, rows, n, rows, pn(0), pr(0), pn(0), pr(0), None, None), "0 patterns"),
                       (lambda: sub(n, rows, n, rows, pn(33), pr(33), pn(33), pr(33), None, None), "33 patterns"),
                       (lambda: sub(n, rows.long(), n, rows, pn(2), pr(2), pn(2), pr(2), None, None), "int32"),
                       (lambda: sub(n, rows, n, rows, pn(2), pr(2).long(), pn(2), pr(2), None, None), "int32"),
                       (lambda: sub(n[:2], rows, n, rows, pn(2), pr(2), pn(2), pr(2), None, None), "one value per row"),
                       (lambda: sub(n, rows, n, rows, pn(3), pr(2), pn(2), pr(2), None, None), "one value per row"),
                       (lambda: sub(n, rows, n, rows, pn(2), pr(2), pn(2), pr(2), u8(2), None), "together"),
                       (lambda: sub(n, rows, n, rows, pn(2), pr(2), pn(2), pr(2), None, u8(2)), "together"),
                       (lambda: sub(n, rows, n, rows, pn(2), pr(2), pn(2), pr(2), u8(3), u8(2)), "one bound per pattern"),
                       (lambda: sub(n, rows, n, rows, pn(2), pr(2), pn(2), pr(2), u8(2), u8(2).int()), "uint8")):
        with pytest.raises(RuntimeError, match=what):
            call()
    assert rec.log == []


def test_public_surface_and_what_the_docstrings_promise():
    assert substructure_map is G.substructure_map and substructure_keep is G.substructure_keep
    assert SubstructureCounts is G.SubstructureCounts
    assert list(inspect.signature(M.substructure_map).parameters) == ["tokens", "patterns", "vocabulary", "device", "normalize"]
    assert list(inspect.signature(M.substructure_keep).parameters) == ["tokens", "patterns", "vocabulary", "device", "occurrences",
                                                                       "normalize", "width", "canonical"]
    assert list(inspect.signature(M.SubstructureCounts).parameters) == ["patterns", "vocabulary", "at_least", "at_most"]
    p = inspect.signature(M.substructure_keep).parameters
    assert (p["occurrences"].default, p["normalize"].default, p["width"].default, p["canonical"].default) == ("all", False, None, False)
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("occurrences", "normalize", "width", "canonical"))
    flat = " ".join(M.substructure_map.__doc__.split())
    for phrase in ("anchors, not atom sets", "not SMARTS", "first map of the lowest found root", "WRITE THE FRAGMENT WITH ITS DISTINCTIVE ATOM FIRST",
                   "4096 steps", "not RDKit's GetSubstructMatches", "lexicographically smallest"):
        assert phrase in flat, phrase
    for doc in (M.substructure_keep.__doc__, M.SubstructureCounts.__doc__, M.screen_tokens_diverse.__doc__):
        for phrase in ("anchors, not atom sets", "not SMARTS"):
            assert phrase in " ".join(doc.split()), (phrase, doc[:60])
    flat = " ".join(M.substructure_keep.__doc__.split())
    for phrase in ("first map of the lowest found root", "AS WRITTEN", "refine_keep_tokens(keep_mask=)", "no kernel of its own"):
        assert phrase in flat, phrase
    assert "substructure_map()" in M.has_substructure.__doc__ and "no mapping is returned" in " ".join(M.has_substructure.__doc__.split())
    assert "``counts``" in M.screen_tokens_diverse.__doc__ and "counts" in M.screen_candidates.__doc__
