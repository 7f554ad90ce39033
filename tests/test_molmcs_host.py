"""No GPU: the definition of mdt_mol_mcs (include/mdt_hip.h) on the plain-int reference tests/molmcs_ref.py -- its size against a
brute force over all entry subsets and injective images, witness validity on every pair of every test, symmetry and spelling
invariance, agreement with the substructure search and the canonical form, the cap figures -- then the shared C++ walk under
AddressSanitizer and UBSan in a stand-alone program (tools/molmcs_host_check.cpp), and the plumbing: C export and argument checks,
op schema and shapes, the launch order of the four Python calls on a recording library, and what the docstrings promise."""
import contextlib
import inspect
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

import molcanon_ref as N
import molkey_ref as K
import molmcs_ref as C
import molsub_ref as B
import smiles_ref as S
from conftest import ROOT
import moleculediffusiontransformer_amd as M
from moleculediffusiontransformer_amd import generative as G, ops, runtime as rt
from moleculediffusiontransformer_amd import McsResult, mcs_keep, mcs_tokens, mol_difference, mol_mcs     # what this file is about

sys.setrecursionlimit(10000)                                                 # (the reference's walk is recursive)

# at most 7 atoms a string: at most 2^8 entry subsets and 7! images a pair
SMALL = ["C", "CC", "CCC", "C1CC1", "C1CC1C", "CC(C)(C)C", "C12CC1C2", "C12C3C1C23", "C.CO", "[NH3+]CC[O-]", "CCO", "C=CC", "C=O",
         "CC(=O)O", "c1ccccc1", "C1CCC1", "N", "CN", "C#N", "OCC", "C1CC1O", "CC=C", "c1ccncc1", "*C*", "C(C)(C)C", "NCCO", "C1=CC=CC=C1"]
CAP_A = "C(C)(C)(C)C(C)(C)C(C)(C)C(C)(C)C(C)(C)C(C)(C)C"
CAP_B = "CC(C)C(C)C(C)C(C)C(C)C(C)C(C)C"


def mcs(a, b, mode=0, **kw):
    """The reference on two strings, and the witness check that every pair of every test goes through"""
    out = C.string_mcs(a, b, mode, **kw)
    (aa, ab), (ba, bb) = C.graph_of(a), C.graph_of(b)
    C.check_witness(out, aa, ab, ba, bb, mode)
    return out


@pytest.fixture(scope="module")
def spelled():
    return K.random_spellings()


# ---------------------------------------------------------------------------------------------------------------------
# the definition on the reference
# ---------------------------------------------------------------------------------------------------------------------
def test_the_size_against_every_entry_subset_under_every_injective_image():
    """Every ordered pair of 27 strings of at most 7 atoms, with and without the floor: the same size as the brute force
    (molmcs_ref.brute_force knows nothing of roots, bounds, floors or steps), and the same winning map either way."""
    assert len(SMALL) >= 25 and all(len(C.graph_of(s)[0]) <= 7 for s in SMALL)
    pairs = 0
    for a in SMALL:
        for b in SMALL:
            (aa, ab), (ba, bb) = C.graph_of(a), C.graph_of(b)
            with_floor, without = mcs(a, b), mcs(a, b, use_floor=False)
            want = C.brute_force(aa, ab, ba, bb)
            assert with_floor["size"] == without["size"] == want, (a, b, with_floor["size"], without["size"], want)
            assert with_floor["map_a"] == without["map_a"] and with_floor["bond_a"] == without["bond_a"], (a, b)
            assert with_floor["steps"] <= without["steps"] and not with_floor["flags"] & C.UNDECIDED
            assert with_floor["search_size"] == with_floor["size"]           # no capped root: the recount is the search's count
            pairs += 1
    assert pairs == 729
    # what an atom-by-atom enumeration with permanent exclusion gets wrong as (2, 3), and the edge kind
    assert mcs("C1CC1C", "CC(C)(C)C")["size"] == (3, 4) and mcs("C1CC1", "CCC")["size"] == (2, 3)
    assert mcs("[NH3+]CC[O-]", "NCCO")["size"] == (3, 4) and mcs("[NH3+]CC[O-]", "NCCO", C.EXACT_ATOMS)["size"] == (1, 2)
    assert mcs("C.CO", "CCO")["size"] == (1, 2) and mcs("C", "N")["flags"] == C.PAIR and mcs("C", "")["flags"] == 0
    exact = [(a, b) for a in SMALL[:12] for b in SMALL[:12]]
    for a, b in exact:                                                       # the other mode, against its own brute force
        (aa, ab), (ba, bb) = C.graph_of(a), C.graph_of(b)
        assert mcs(a, b, C.EXACT_ATOMS)["size"] == C.brute_force(aa, ab, ba, bb, C.EXACT_ATOMS), (a, b)


def test_symmetry_spelling_invariance_and_the_whole_flags(spelled):
    """The size is symmetric in A and B and the same under every spelling of either side; two spellings of one connected graph are
    all of each other under `exact`; and where a pair is all of each other with equal counts, the canonical form says same."""
    pairs, most, steps = 0, 0, 0
    for k in range(0, 58, 2):
        (ga, sa), (gb, sb) = spelled[k], spelled[k + 1]
        sizes = set()
        for i, j in ((0, 0), (1, 2), (3, 1), (2, 3)):
            ab, ba = mcs(sa[i], sb[j]), mcs(sb[j], sa[i])
            assert not (ab["flags"] | ba["flags"]) & C.UNDECIDED
            sizes |= {ab["size"], ba["size"]}
            most = max([most] + [r[4] for r in ab["roots"] + ba["roots"]])
            steps += ab["steps"] + ba["steps"]
            pairs += 2
        assert len(sizes) == 1, (sa, sb, sizes)
    assert (pairs, most, steps) == (232, 21, 1911), (pairs, most, steps)      # the reference's own figures: at most 21 steps a root
    same = 0
    for g, sp in spelled[:60]:
        out = mcs(sp[0], sp[3], C.EXACT_ATOMS)
        connected = len(g.components()) == 1
        whole = C.WHOLE_A | C.WHOLE_B
        assert (out["flags"] & whole == whole) == connected, sp
        assert out["size"] == (len(g.bonds), len(g.atoms)) or not connected
        same += connected
    assert same == 33
    agreed = checked = 0
    strings = [sp[k % 4] for k, (_, sp) in enumerate(spelled[:40])] + SMALL
    for a in strings[::3]:
        for b in strings[1::3] + [a]:
            out = mcs(a, b, C.EXACT_ATOMS)
            (aa, ab), (ba, bb) = C.graph_of(a), C.graph_of(b)
            both = out["flags"] & (C.WHOLE_A | C.WHOLE_B) == C.WHOLE_A | C.WHOLE_B and (len(aa), len(ab)) == (len(ba), len(bb))
            if aa and ba and len(N.components(len(aa), ab)) == 1:
                assert both == (N.form(N.string_canon(a)) == N.form(N.string_canon(b))), (a, b)
                agreed, checked = agreed + both, checked + 1
    assert (checked, agreed) == (368, 18)


def test_all_of_a_exactly_when_the_substructure_search_finds_it(spelled):
    """Unbracketed, connected, '*'-free patterns against the spellings: WHOLE_A is mdt_sub_match's match"""
    patterns = [p for p in B.PATTERNS + B.EVERYDAY if not set(p) & set("[.*")]
    targets = [sp[k % 4] for k, (_, sp) in enumerate(spelled[:70])]
    hits = pairs = 0
    for p in dict.fromkeys(patterns):
        for t in targets:
            out = mcs(p, t)
            assert not out["flags"] & C.UNDECIDED
            found = bool(out["flags"] & C.WHOLE_A)
            assert found == B.contains(p, t), (p, t, out["size"])
            hits, pairs = hits + found, pairs + 1
    assert (pairs, hits) == (1400, 295), (pairs, hits)                       # 20 patterns x 70 targets: the reference's own figures


def test_the_cap():
    """The figures the definition gave before anything was built: 7 capped roots of 320 and the lower bound (13, 14) on a pair of
    branched alkanes; 4,096 roots, 8,002 steps and none capped on 64 stars."""
    out = mcs(CAP_A, CAP_B)
    assert len(out["roots"]) == 320 and sum(r[5] for r in out["roots"]) == 7 and out["size"] == (13, 14) and out["flags"] & C.UNDECIDED
    assert all(r[4] == C.MAX_STEPS for r in out["roots"] if r[5]) and all(r[4] <= C.MAX_STEPS for r in out["roots"])
    assert out["steps"] == sum(r[4] for r in out["roots"]) == 78661 and out["floor"] == (5, 6)
    stars = mcs("*" * 64, "*" * 64)
    assert len(stars["roots"]) == 4096 and stars["size"] == (63, 64) and stars["steps"] == 8002 and not stars["flags"] & C.UNDECIDED
    assert max(r[4] for r in stars["roots"]) == 126 and stars["flags"] == C.PAIR | C.COMMON | C.WHOLE_A | C.WHOLE_B
    low = mcs(CAP_A, CAP_B, cap=50)                                          # a lower cap: still a witness, never a greater size
    assert low["flags"] & C.UNDECIDED and low["size"] <= out["size"] and low["steps"] <= 50 * 320


# ---------------------------------------------------------------------------------------------------------------------
# the shared C++ walk on the host, under AddressSanitizer and UBSan
# ---------------------------------------------------------------------------------------------------------------------
def test_the_host_program_agrees_with_the_reference_under_the_sanitizers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import molmcs_host_rows
    rows, exe = str(tmp_path / "rows.txt"), str(tmp_path / "molmcs_host_check")
    pairs = molmcs_host_rows.main(rows, graphs=30)
    subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "molmcs_host_check.cpp"), "-o", exe], check=True, capture_output=True, text=True)
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
    assert re.search(r"\bint mdt_mol_mcs\s*\(", hdr) and "mdt_mol_mcs" in rt.SYMBOLS and hasattr(lib, "mdt_mol_mcs")
    assert len(rt.SYMBOLS["mdt_mol_mcs"][1]) == 24
    assert int(re.search(r"#define MDT_ABI_VERSION (\d+)", hdr).group(1)) == rt.ABI_VERSION == 5 == lib.mdt_abi_version()
    assert int(re.search(r"#define MDT_MCS_MAX_STEPS (\d+)", hdr).group(1)) == rt.MCS_MAX_STEPS == C.MAX_STEPS
    assert (rt.MCS_EXACT_ATOMS, rt.MCS_PAIR, rt.MCS_COMMON, rt.MCS_UNDECIDED, rt.MCS_WHOLE_A, rt.MCS_WHOLE_B) == \
        (C.EXACT_ATOMS, C.PAIR, C.COMMON, C.UNDECIDED, C.WHOLE_A, C.WHOLE_B)
    flat = " ".join(hdr.replace(" * ", " ").split())
    for phrase in ("Not RDKit's FindMCS", "no ring-matches-ring options", "no SMARTS result", "No stereo", "ONE fragment",
                   "Aromaticity is as handed in", "bonds first", "edge kind, not the induced kind", "GREEDY DESCENT", "ties to the lowest root",
                   "RECOUNTED from M", "4,096 roots of 4,096 steps", "every word is the same under any scheduling", "0x7FF"):
        assert phrase in flat, phrase
    src = open(os.path.join(ROOT, "moleculediffusiontransformer_amd", "csrc", "k_molmcs.hip")).read()
    assert "mcs_root_walk(" in src and "mcs_root_greedy(" in src and "k_mol_mcs" in src     # the kernel runs the walk the host check runs
    shared = open(os.path.join(ROOT, "moleculediffusiontransformer_amd", "csrc", "mdt_molmcs.h")).read()
    assert "mcs_root_walk(" in shared and "mcs_pair(" in shared and "mcs_root_greedy(" in shared
    from moleculediffusiontransformer_amd import build as b
    assert ("k_molmcs.hip", []) in b.SOURCES


def test_entry_point_refuses_bad_arguments_before_any_launch():
    lib = rt.load_library()

    def call(LA=32, R_=5, LB=8, RB=5, mode=0, a=8, b=8, out=8):
        return lib.mdt_mol_mcs(a, a, a, a, LA, R_, b, b, b, b, LB, RB, mode, out, out, out, out, out, out, out, out, out, out, 0)
    for kw, what in ((dict(LA=0), b"LA <= 64"), (dict(LA=65), b"LA <= 64"), (dict(LB=0), b"LB <= 64"), (dict(LB=65), b"LB <= 64"),
                     (dict(R_=-1, RB=-1), b"R >= 0"), (dict(RB=4), b"RB == R"), (dict(RB=0), b"RB == R"), (dict(mode=2), b"mode"),
                     (dict(mode=3), b"mode"), (dict(mode=-1), b"mode"), (dict(a=0), b"null"), (dict(b=0), b"null"), (dict(out=0), b"null")):
        assert call(**kw) == 2, kw
        assert what in lib.mdt_last_error(), (kw, lib.mdt_last_error())
    assert call(R_=0, RB=0) == 0 and call(R_=0, RB=1, a=0, b=0, out=0) == 0   # nothing to do: nothing launched or read
    assert call(R_=0, RB=0, mode=2) != 0 and call(R_=0, RB=2) != 0            # ... but a bad argument is still one


def vocabulary():
    return M.SmilesVocabulary([None] + S.CHARS)


def test_op_schema_and_shape_inference():
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert str(torch.ops.mdt.mol_mcs.default._schema) == \
        ("mdt::mol_mcs(Tensor a_natoms, Tensor a_atoms, Tensor a_nbonds, Tensor a_bonds, Tensor b_natoms, Tensor b_atoms, "
         "Tensor b_nbonds, Tensor b_bonds, SymInt mode) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)")
    with FakeTensorMode():
        n, rows = torch.empty(15, dtype=torch.int32), torch.empty(15, 40, dtype=torch.int32)
        for RB in (15, 1):
            bn, brows = torch.empty(RB, dtype=torch.int32), torch.empty(RB, 9, dtype=torch.int32)
            out = torch.ops.mdt.mol_mcs(n, rows, n, rows, bn, brows, bn, brows, 1)
            assert [(tuple(t.shape), t.dtype) for t in out] == [
                ((15, 2), torch.int32), ((15, 40), torch.uint8), ((15,), torch.int64), ((15,), torch.int32), ((15,), torch.int32),
                ((15, 40), torch.int32), ((15,), torch.int32), ((15, 40), torch.int32), ((15, 40), torch.uint8), ((15,), torch.uint8)]
    n, rows = torch.zeros(3, dtype=torch.int32), torch.zeros(3, 4, dtype=torch.int32)       # no CPU implementation behind the op
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        torch.ops.mdt.mol_mcs(n, rows, n, rows, n, rows, n, rows, 0)


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


R_, LA_, LB_ = 15, 16, 11
GRAPH = ["mdt_tokens_compact", "mdt_mol_graph"]
NORMAL_FORM = ["mdt_mol_hydrogens", "mdt_mol_rings", "mdt_mol_normalize"]


def names(rec):
    return [e[0] for e in rec.log]


def test_launch_order_of_the_four_public_calls(rec):
    a, b, one, v = torch.ones(R_, LA_, dtype=torch.long), torch.ones(R_, LB_, dtype=torch.int16), torch.ones(1, LB_, dtype=torch.long), vocabulary()
    out = mol_mcs(a, b, v, "cpu")
    assert names(rec) == GRAPH + GRAPH + ["mdt_mol_mcs"]
    ga, gb, call = rec.log[1], rec.log[3], rec.log[4]
    assert len(call) == 1 + 24 and call[1:5] == ga[8:12] and call[7:11] == gb[8:12] and call[5:7] == (LA_, R_) and call[11:14] == (LB_, R_, 0)
    assert all(call[14:24]) and len(set(call[14:24])) == 10                  # every output, each its own
    assert isinstance(out, McsResult) and out._fields == (
        "bonds", "atoms", "map_a", "in_a", "in_b", "similarity", "undecided", "whole_a", "whole_b", "steps", "natoms", "graph_atoms",
        "nbonds", "graph_bonds", "atom_map", "pair", "a_status", "a_position", "b_status", "b_position")
    assert [(tuple(t.shape), t.dtype) for t in out] == [
        ((R_,), torch.int64), ((R_,), torch.int64), ((R_, LA_), torch.int64), ((R_, LA_), torch.bool), ((R_, LB_), torch.bool),
        ((R_,), torch.float64), ((R_,), torch.bool), ((R_,), torch.bool), ((R_,), torch.bool), ((R_,), torch.int64), ((R_,), torch.int64),
        ((R_, LA_), torch.int64), ((R_,), torch.int64), ((R_, LA_), torch.int64), ((R_, LA_), torch.int64), ((R_,), torch.bool),
        ((R_,), torch.int64), ((R_,), torch.int64), ((R_,), torch.int64), ((R_,), torch.int64)]
    assert not out.similarity.any()                                          # no pair anywhere (the recorder writes nothing): 0, not NaN
    rec.log.clear()
    out = mol_mcs(a, one, v, "cpu", normalize=True, atoms="exact")           # one b row; the normal forms are what is matched
    assert names(rec) == GRAPH + NORMAL_FORM + GRAPH + NORMAL_FORM + ["mdt_mol_mcs"]
    na, nb, call = rec.log[4], rec.log[9], rec.log[10]
    assert (call[2], call[4]) == (na[11], na[12]) and (call[8], call[10]) == (nb[11], nb[12]) and call[11:14] == (LB_, 1, 1)
    assert out.in_b.shape == (R_, LB_) and out.b_status.shape == (1,)
    rec.log.clear()
    only_a, only_b, undecided = mol_difference(a, b, v, "cpu")
    assert names(rec) == GRAPH + GRAPH + ["mdt_mol_mcs"]
    assert [(tuple(t.shape), t.dtype) for t in (only_a, only_b, undecided)] == [((R_, LA_), torch.bool), ((R_, LB_), torch.bool), ((R_,), torch.bool)]
    rec.log.clear()
    out = mcs_tokens(a, b, v, "cpu", width=20)
    assert names(rec) == GRAPH + GRAPH + ["mdt_mol_mcs", "mdt_mol_rank", "mdt_mol_write"]
    call, rank, write = rec.log[4], rec.log[5], rec.log[6]
    assert write[1:5] == rank[1:5] == call[18:22]                             # the writer takes the op's own graph arrays
    assert [(tuple(t.shape), t.dtype) for t in out] == [((R_, 20), torch.int64), ((R_,), torch.int64), ((R_,), torch.bool),
                                                        ((R_,), torch.int64), ((R_,), torch.int64)]
    rec.log.clear()
    assert mcs_tokens(a, one, v, "cpu", canonical=True)[0].shape == (R_, LA_)
    assert names(rec) == GRAPH + GRAPH + ["mdt_mol_mcs", "mdt_mol_rank", "mdt_mol_canon", "mdt_mol_write"]
    # mcs_keep(): the mask is torch on the ops' outputs; with normalize the match reads the normal forms and the writer the lead's
    # graph as written
    rec.log.clear()
    out = mcs_keep(a, b, v, "cpu", width=24)
    assert names(rec) == GRAPH + GRAPH + ["mdt_mol_mcs", "mdt_mol_rank", "mdt_mol_write"]
    assert rec.log[6][1:5] == rec.log[1][8:12]                               # the lead's own graph is written
    assert [(tuple(t.shape), t.dtype) for t in out] == [((R_, 24), torch.int64), ((R_, 24), torch.bool), ((R_,), torch.bool),
                                                        ((R_,), torch.int64), ((R_,), torch.int64), ((R_,), torch.int64)]
    rec.log.clear()
    mcs_keep(a, one, v, "cpu", normalize=True, canonical=True)
    assert names(rec) == GRAPH + NORMAL_FORM + GRAPH + NORMAL_FORM + ["mdt_mol_mcs", "mdt_mol_rank", "mdt_mol_canon", "mdt_mol_write"]
    graph, normal, call, write = rec.log[1], rec.log[4], rec.log[10], rec.log[13]
    assert (call[2], call[4]) == (normal[11], normal[12]) and write[1:5] == graph[8:12] and call[2] != graph[9]


def test_refusals_come_before_anything_is_launched(rec):
    v = vocabulary()
    a, b = torch.ones(R_, LA_, dtype=torch.long), torch.ones(R_, LB_, dtype=torch.long)
    wide = torch.ones(R_, 65, dtype=torch.long)
    for f in (mol_mcs, mol_difference, mcs_tokens, mcs_keep):
        for call, what in ((lambda: f(a, b[:4], v, "cpu"), "row by row"),
                           (lambda: f(a, b[:0], v, "cpu"), "row by row"),
                           (lambda: f(a, b, v, "cpu", atoms="charge"), "atoms must be one of"),
                           (lambda: f(a, b, v, "cpu", atoms=None), "atoms must be one of"),
                           (lambda: f(a, b, v, "cpu", normalize=1), "normalize must be"),
                           (lambda: f(a, b, S.CHARS, "cpu"), "SmilesVocabulary"),
                           (lambda: f(wide, b, v, "cpu"), "1 to 64"),
                           (lambda: f(a, wide, v, "cpu"), "1 to 64"),
                           (lambda: f(a, b[:, :0], v, "cpu"), "1 to 64"),
                           (lambda: f(a.float(), b, v, "cpu"), "integer"),
                           (lambda: f(a, b.float(), v, "cpu"), "integer")):
            with pytest.raises(ValueError, match=what):
                call()
    for f in (mcs_tokens, mcs_keep):
        for call, what in ((lambda: f(a, b, v, "cpu", width=129), "width"), (lambda: f(a, b, v, "cpu", width=0), "width"),
                           (lambda: f(a, b, v, "cpu", canonical=1), "canonical")):
            with pytest.raises(ValueError, match=what):
                call()
    assert rec.log == []
    # the op refuses what the kernel does not take
    n, rows = torch.zeros(3, dtype=torch.int32), torch.zeros(3, 8, dtype=torch.int32)
    big = torch.zeros(3, 65, dtype=torch.int32)
    op = torch.ops.mdt.mol_mcs
    for call, what in ((lambda: op(n, big, n, big, n, rows, n, rows, 0), "1 to 64"),
                       (lambda: op(n, rows, n, rows, n, big, n, big, 0), "1 to 64"),
                       (lambda: op(n, rows.long(), n, rows, n, rows, n, rows, 0), "int32"),
                       (lambda: op(n, rows, n, rows, n, rows, n.long(), rows, 0), "int32"),
                       (lambda: op(n[:2], rows, n, rows, n, rows, n, rows, 0), "one value per row"),
                       (lambda: op(n, rows, n, rows, n, rows, n[:1], rows, 0), "one value per row"),
                       (lambda: op(n, rows, n, rows, n[:2], rows[:2], n[:2], rows[:2], 0), "2 rows"),
                       (lambda: op(n, rows, n, rows, n, rows, n, rows, 2), "mode"),
                       (lambda: op(n, rows, n, rows, n, rows, n, rows, 3), "mode"),
                       (lambda: op(n, rows, n, rows[:, :4], n, rows, n, rows, 0), "int32")):
        with pytest.raises(RuntimeError, match=what):
            call()
    assert rec.log == []
    op(n[:0], rows[:0], n[:0], rows[:0], n[:1], rows[:1], n[:1], rows[:1], 0)   # no rows: nothing is launched
    assert rec.log == []


def test_public_surface_and_what_the_docstrings_promise():
    assert mol_mcs is G.mol_mcs and mol_difference is G.mol_difference and mcs_tokens is G.mcs_tokens and mcs_keep is G.mcs_keep
    assert list(inspect.signature(M.mol_mcs).parameters) == ["a_tokens", "b_tokens", "vocabulary", "device", "normalize", "atoms"]
    assert list(inspect.signature(M.mol_difference).parameters) == ["a_tokens", "b_tokens", "vocabulary", "device", "normalize", "atoms"]
    assert list(inspect.signature(M.mcs_tokens).parameters) == ["a_tokens", "b_tokens", "vocabulary", "device", "normalize", "atoms",
                                                                "width", "canonical"]
    assert list(inspect.signature(M.mcs_keep).parameters) == ["lead_tokens", "other_tokens", "vocabulary", "device", "normalize", "atoms",
                                                              "width", "canonical"]
    for f in (M.mol_mcs, M.mol_difference, M.mcs_tokens, M.mcs_keep):
        p = inspect.signature(f).parameters
        assert (p["normalize"].default, p["atoms"].default) == (False, "element")
        assert all(q.kind is inspect.Parameter.KEYWORD_ONLY for name, q in p.items() if name in ("normalize", "atoms", "width", "canonical"))
    assert G.MCS_ATOMS == ("element", "exact")
    flat = " ".join(M.mol_mcs.__doc__.split())
    for phrase in ("not RDKit's FindMCS", "bonds first", "edge kind, not the induced kind", "4096 steps", "LOWER bound", "ONE fragment",
                   "no stereo", "Sequence: mdt::tokens_compact -> mdt::mol_graph", "then mdt::mol_mcs", "mdt_mol_mcs in include/mdt_hip.h",
                   "from the exact integer counts", "ONE row", "ValueError before anything is launched"):
        assert phrase in flat, phrase
    flat = " ".join(M.mcs_keep.__doc__.split())
    for phrase in ("AS WRITTEN", "refine_keep_tokens(keep_mask=)", "no kernel of its own", "substructure_keep()", "mdt::mol_mcs",
                   "mdt::mol_write", "not RDKit's FindMCS"):
        assert phrase in flat, phrase
    assert "view_difference()" in M.mol_difference.__doc__ and "Sequence: mol_mcs()'s" in " ".join(M.mol_difference.__doc__.split())
    flat = " ".join(M.mcs_tokens.__doc__.split())
    assert "mdt::mol_rank -> mdt::mol_canon (only with ``canonical=True``) -> mdt::mol_write" in flat and "NOT RDKit's canonical SMILES" in flat
