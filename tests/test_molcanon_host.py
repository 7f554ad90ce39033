"""No GPU: the definition of the canonical atom order (include/mdt_hip.h, mdt_mol_canon) on its reference (tests/molcanon_ref.py) --
symmetric molecules and coronene under renumbering, the leaf and node counts of the search trees, components, the node cap,
exactness against a brute-force canoniser, the random spellings, the edges -- and the plumbing: the C export and its argument
checks, the enumerators, the op schema and shape inference, the launch order of the public calls with canonical=True on a recording
library, and the refusals."""
import contextlib
import itertools
import os
import random
import re

import pytest
import torch

import molcanon_ref as Q
import molkey_ref as K
import molwrite_ref as W
import smiles_ref as S
from conftest import ROOT
import moleculediffusiontransformer_amd as M
from moleculediffusiontransformer_amd import ops, runtime as rt

# the 30 symmetric molecules of test_molwrite_host.py
SYMMETRIC = ["C12C3C4C1C5C2C3C45", "C12C3C1C1C4C2C3C41", "C12C3C1C1C2C31", "C1C2CC3CC1CC(C2)C3", "c1ccc(cc1)-c1ccccc1", "c1ccc2ccccc2c1",
             "c1ccc2cc3ccccc3cc2c1", "c1cc2ccc3cccc4ccc(c1)c2c34", "C1CCC2(CC1)CCCCC2", "C1CC2CCC1C2", "C1CC2CCC1CC2",
             "OC(=O)CC(O)(CC(O)=O)C(O)=O", "C1CC1.C1CC1", "C12C3C4C1C5C2C3C45.C12C3C4C1C5C2C3C45",
             "c1ccccc1", "C1CCCCC1", "CC(C)(C)C", "C1CC1", "C12C3C1C23", "Cc1cc(C)cc(C)c1", "Cc1ccc(C)cc1", "ClC(Cl)(Cl)Cl",
             "FC(F)(F)C(F)(F)F", "O=C=O", "C1COCCO1", "C1CCC2CCCCC2C1", "C1CCCCC1C1CCCCC1", "CC.CC.CC", "c1ccc2c(c1)c1ccccc1c1ccccc21",
             "[NH4+].[Cl-].[NH4+].[Cl-]"]
CORONENE = "c1cc2ccc3ccc4ccc5ccc6ccc1c1c2c3c4c5c61"
CUBANE, ADAMANTANE = "C12C3C4C1C5C2C3C45", "C1C2CC3CC1CC(C2)C3"
DODECAHEDRANE = "C12C3C4C5C1C1C6C2C2C3C3C4C4C5C1C1C6C2C3C41"
HEXAPHENYLBENZENE = "c1ccccc1c1c(c2ccccc2)c(c2ccccc2)c(c2ccccc2)c(c2ccccc2)c1c1ccccc1"
HEXAPHENYLETHANE = "c1ccccc1C(c1ccccc1)(c1ccccc1)C(c1ccccc1)(c1ccccc1)c1ccccc1"
PERFLUOROHEXANE = "FC(F)(F)C(F)(F)C(F)(F)C(F)(F)C(F)(F)C(F)(F)F"
# molecule: (leaves, nodes).  The leaves follow from the symmetry; the nodes are what this reference gives (they depend on which
# class has the smallest label value)
TREES = {"c1ccccc1": (12, 19), CUBANE: (48, 81), ADAMANTANE: (24, 41), CORONENE: (12, 19), DODECAHEDRANE: (120, 201),
         "CC(C)(C)C": (1, 1), PERFLUOROHEXANE: (2, 3), HEXAPHENYLBENZENE: (768, 1531)}


@pytest.fixture(scope="module")
def spelled():
    return K.random_spellings()


def renumbered(atoms, bonds, rng):
    """The same graph under a random numbering of its atoms, a random order of its entries and random orientations."""
    to = list(range(len(atoms)))
    rng.shuffle(to)
    new_atoms = [0] * len(atoms)
    for a, d in enumerate(atoms):
        new_atoms[to[a]] = d
    new_bonds = [(to[a], to[b], o) if rng.random() < 0.5 else (to[b], to[a], o) for a, b, o in bonds]
    rng.shuffle(new_bonds)
    return new_atoms, new_bonds


def arrays_canon(atoms, bonds, width=Q.MAX_WIDTH):
    return Q.canon(len(atoms), atoms, len(bonds), bonds, width)


# ---------------------------------------------------------------------------------------------------------------------
# the definition on the reference
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", SYMMETRIC + [CORONENE])
def test_a_symmetric_molecule_has_one_form_and_one_row_under_renumbering(s):
    status, _, atoms, bonds = K.graph(s)
    assert status == 0
    rng = random.Random(len(s))
    forms, rows = set(), set()
    for _ in range(24):
        new_atoms, new_bonds = renumbered(atoms, bonds, rng)
        out = arrays_canon(new_atoms, new_bonds)
        assert out["flags"] == Q.CANONICAL and out["nodes"] < 2 * out["leaves"]
        assert sorted(out["priority"][:len(atoms)]) == list(range(1, len(atoms) + 1)) and not any(out["priority"][len(atoms):])
        forms.add(Q.form(out))
        rows.add(Q.graph_write(new_atoms, new_bonds, W.ASCII_CLASS_ID)["text"])
    assert forms == {Q.form(Q.string_canon(s))} and len(rows) == 1 and K.string_key(min(rows)) == K.string_key(s), rows


def test_coronene_is_one_row_with_the_search_and_more_without():
    assert len(SYMMETRIC) == len(set(SYMMETRIC)) == 30
    _, _, atoms, bonds = K.graph(CORONENE)
    rng = random.Random(11)
    numberings = [renumbered(atoms, bonds, rng) for _ in range(24)]
    searched = {Q.graph_write(a, b, W.ASCII_CLASS_ID)["text"] for a, b in numberings}
    ranked = {W.graph_write(a, b, W.ASCII_CLASS_ID, 128)["text"] for a, b in numberings}
    print("coronene: %d row with the search, %d with mdt_mol_rank's priority" % (len(searched), len(ranked)))
    assert len(searched) == 1 and len(ranked) > 1                            # the same loop without the search: the test bites


@pytest.mark.parametrize("s", sorted(TREES))
def test_the_leaves_and_nodes_of_the_search_trees(s):
    out = Q.string_canon(s)
    print("%s: %d leaves, %d nodes" % (s, out["leaves"], out["nodes"]))
    assert (out["flags"], out["leaves"], out["nodes"]) == (Q.CANONICAL,) + TREES[s] and out["nodes"] < 2 * out["leaves"]
    assert len(K.graph(HEXAPHENYLBENZENE)[2]) == 42 and len(HEXAPHENYLBENZENE) == 64


def test_components_are_searched_one_by_one():
    two, one = Q.string_canon(CUBANE + "." + CUBANE), Q.string_canon(CUBANE)
    assert two["nodes"] == 2 * one["nodes"] == 162 and two["leaves"] == 2 * one["leaves"]       # the sum, not the product
    assert two["canon_atoms"][:16] == one["canon_atoms"][:8] * 2 and sorted(two["priority"][:16]) == list(range(1, 17))
    assert two["canon_bonds"][12:24] == [w + (8 | 8 << 8) for w in two["canon_bonds"][:12]]     # one component after the other, alike
    assert all((w & 255) < 8 and (w >> 8 & 255) < 8 for w in two["canon_bonds"][:12]) and not any(two["canon_bonds"][24:])
    ions = Q.string_canon(".".join(["[Cl-]"] * 8))
    assert (ions["flags"], ions["nodes"], ions["leaves"]) == (Q.CANONICAL, 8, 8) and ions["priority"][:8] == list(range(1, 9))
    _, _, atoms, bonds = K.graph("CC.CC.CC")
    rng = random.Random(2)
    assert len({Q.form(arrays_canon(*renumbered(atoms, bonds, rng))) for _ in range(24)}) == 1
    mixed = Q.string_canon("CCO.C.CC")                                       # ascending certificate: the sizes lead
    c, o = K.descriptor("C"), K.descriptor("O")
    assert mixed["canon_atoms"][:6] in ([c, c, c, c, c, o], [c, c, c, c, o, c], [c, c, c, o, c, c]) and mixed["priority"][3] == 1
    ends = [(w & 255, w >> 8 & 255) for w in mixed["canon_bonds"][:3]]
    assert ends[0] == (1, 2) and all(3 <= lo < hi <= 5 for lo, hi in ends[1:]) and ends == sorted(ends)


def test_a_row_above_the_cap_is_undecided():
    status, _, atoms, bonds = K.graph(HEXAPHENYLETHANE)
    assert (status, len(HEXAPHENYLETHANE), len(atoms), len(bonds)) == (0, 58, 38, 43)
    out = Q.string_canon(HEXAPHENYLETHANE)
    assert out["flags"] == Q.UNDECIDED and out["nodes"] > Q.MAX_NODES
    assert not any(out["priority"]) and not any(out["canon_atoms"]) and not any(out["canon_bonds"])
    assert Q.respell(HEXAPHENYLETHANE) == W.respell(HEXAPHENYLETHANE) != ""  # written with mdt_mol_rank's priority
    small = Q.canon(8, [K.descriptor("C")] * 8, 12, K.graph(CUBANE)[3], 64, max_nodes=80)      # the cap is on the nodes: cubane has 81
    assert small["flags"] == Q.UNDECIDED and Q.canon(8, [K.descriptor("C")] * 8, 12, K.graph(CUBANE)[3], 64, max_nodes=81)["flags"] == Q.CANONICAL


def test_exactness_against_brute_force():
    """Random graphs of at most 7 atoms, and all their pairs: equal canonical arrays exactly when the brute-force certificates are
    equal."""
    rng = random.Random(19)
    graphs = []
    while len(graphs) < 220:
        g = K.random_graph(rng, 7)
        if len(g.atoms) <= 7:
            graphs.append((g.descriptors(), list(g.bonds)))
    graphs += [renumbered(a, b, rng) for a, b in graphs[:60]]                # pairs that ARE equal, numbered differently
    forms = [(len(a), len(b)) + Q.form(arrays_canon(a, b, 8)) for a, b in graphs]
    brutes = [Q.brute(a, b) for a, b in graphs]
    keys = [K.key(a, b) for a, b in graphs]
    assert all(arrays_canon(a, b, 8)["flags"] == Q.CANONICAL for a, b in graphs)
    equal = 0
    for i, j in itertools.combinations(range(len(graphs)), 2):
        assert (forms[i] == forms[j]) == (brutes[i] == brutes[j]), (graphs[i], graphs[j])
        equal += forms[i] == forms[j]
    print("%d graphs: %d distinct forms, %d distinct keys, %d equal pairs" % (len(graphs), len(set(forms)), len(set(keys)), equal))
    assert len(graphs) >= 150 and equal >= 60 and len(set(forms)) == len(set(brutes)) >= 100


def test_the_random_spellings(spelled):
    decided = one = back = fixed = 0
    for g, sp in spelled:
        forms = set()
        for s in sp:
            _, _, atoms, bonds = K.graph(s)
            out = arrays_canon(atoms, bonds)
            decided += out["flags"] == Q.CANONICAL and out["nodes"] < 2 * out["leaves"]
            forms.add(Q.form(out))
            text = Q.respell(s)
            back += K.string_key(text) == K.string_key(s) != 0
            fixed += Q.respell(text) == text
        one += len(forms) == 1 and len({Q.respell(s) for s in sp}) == 1
    print("decided %d, one form and one row %d, read back %d, fixed points %d" % (decided, one, back, fixed))
    assert (decided, one, back, fixed) == (2000, 500, 2000, 2000)


def test_the_edges():
    """The edge arrays on the Python restatement of the serial form.  The C++ serial form itself (molc_row, csrc/mdt_molcanon.h) is
    asked the same rows (molcanon_ref.edge_rows()) by tools/molcanon_host_check.cpp, a stand-alone program that this suite does not
    build; the kernel is asked them in tests/test_gpu_molcanon.py."""
    rows = {(w, n, nb): (atoms, bonds) for w, n, nb, atoms, bonds in Q.edge_rows()}
    answer = lambda w, n, nb: Q.canon(n, rows[w, n, nb][0], nb, rows[w, n, nb][1], w)  # noqa: E731
    one = answer(8, 1, 0)
    assert (one["flags"], one["nodes"], one["priority"], one["canon_atoms"][0]) == (1, 1, [1] + [0] * 7, K.descriptor("C")) and not any(one["canon_bonds"])
    chain, ring = answer(64, 64, 63), answer(64, 64, 64)
    assert (chain["flags"], chain["leaves"], chain["nodes"]) == (1, 2, 3) and (ring["flags"], ring["leaves"], ring["nodes"]) == (1, 128, 193)
    assert sorted(ring["priority"]) == list(range(1, 65)) and len(set(ring["canon_bonds"])) == 64
    cf4 = answer(8, 5, 4)
    assert (cf4["flags"], cf4["nodes"]) == (1, 1)                            # all twins: nothing to search
    rng = random.Random(4)
    for at in ((8, 3, 3), (8, 4, 5), (8, 4, 0)):                             # an entry (a, a); a pair named twice; no entries
        atoms, bonds = rows[at]
        out = answer(*at)
        assert out["flags"] == Q.CANONICAL and out["nodes"] < 2 * out["leaves"]
        for _ in range(12):
            new_atoms, new_bonds = renumbered(atoms, bonds, rng)
            assert Q.form(Q.canon(at[1], new_atoms, at[2], new_bonds, 8)) == Q.form(out), at
    for at in ((8, 0, 0), (8, 9, 0), (8, 3, 9), (8, 3, 2)):                  # counts out of range, an end beyond n: all zero
        out = answer(*at)
        assert out["flags"] == 0 and out["nodes"] == 0 and not any(out["priority"] + out["canon_atoms"] + out["canon_bonds"]), at


# ---------------------------------------------------------------------------------------------------------------------
# the plumbing
# ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_the_library_exports_the_new_symbol():
    hdr = open(os.path.join(ROOT, "include", "mdt_hip.h")).read()
    lib = rt.load_library()
    assert re.search(r"\bint mdt_mol_canon\s*\(", hdr) and "mdt_mol_canon" in rt.SYMBOLS and hasattr(lib, "mdt_mol_canon")
    assert len(rt.SYMBOLS["mdt_mol_canon"][1]) == 12
    assert int(re.search(r"#define MDT_ABI_VERSION (\d+)", hdr).group(1)) == rt.ABI_VERSION == 5 == lib.mdt_abi_version()
    for name, value in (("CANONICAL", Q.CANONICAL), ("UNDECIDED", Q.UNDECIDED)):
        assert int(re.search(r"\bMDT_MOLC_%s = (\d+)" % name, hdr).group(1)) == value == getattr(rt, "MOLC_" + name)
    assert int(re.search(r"\bMDT_MOLC_MAX_NODES = (\d+)", hdr).group(1)) == Q.MAX_NODES == rt.MOLC_MAX_NODES
    flat = " ".join(hdr.replace(" * ", " ").split())
    for phrase in ("lab[m_j] = mix(mix(atoms[m_j]) ^ (ROOT + j))", "TWIN CLASS", "the smallest label value", "never on a hash of them",
                   "ascending (certificate, lowest atom index)", "nodes < 2 x leaves", "RDKit's canonical SMILES", "a marked atom stands alone"):
        assert phrase in flat, phrase
    assert "k_molcanon.hip" in [s for s, _ in __import__("moleculediffusiontransformer_amd.build", fromlist=["SOURCES"]).SOURCES]
    csrc = os.path.join(ROOT, "moleculediffusiontransformer_amd", "csrc")
    src, shared = open(os.path.join(csrc, "k_molcanon.hip")).read(), open(os.path.join(csrc, "mdt_molcanon.h")).read()
    for used in ("molc_refine(", "molc_target(", "molc_twin_key(", "mol_graph_ok_wave(", "mdt_molcanon.h", "mdt_finish(", "__ballot("):
        assert used in src, used
    scan = open(os.path.join(csrc, "mdt_smiles_scan.h")).read()
    assert "molc_row(" in shared and "uint64_t mol_root_hash(" not in src + shared and scan.count("uint64_t mol_root_hash(") == 1
    for f in (M.mol_write, M.mol_respell, M.scaffold_tokens, M.scaffold_keep, M.mol_canon):
        doc = " ".join(f.__doc__.split())
        assert "RDKit's canonical" in doc and ("canonical=True" in doc or f is M.mol_canon), f.__name__
    readme = " ".join(open(os.path.join(ROOT, "README.md")).read().split())
    assert "mol_canon" in readme and "mol_same" in readme and "canonical=True" in readme


def test_the_entry_point_refuses_bad_arguments_before_any_launch():
    lib = rt.load_library()

    def canon(L=32, R_=5, p=8, out=8, **one):
        a = dict(natoms=p, atoms=p, nbonds=p, bonds=p, priority=out, canon_atoms=out, canon_bonds=out, nodes=out, flags=out)
        a.update(one)
        return lib.mdt_mol_canon(a["natoms"], a["atoms"], a["nbonds"], a["bonds"], L, R_, a["priority"], a["canon_atoms"], a["canon_bonds"],
                                 a["nodes"], a["flags"], 0)
    cases = [(dict(L=0), b"L <= 64"), (dict(L=65), b"L <= 64"), (dict(R_=-1), b"R >= 0"), (dict(p=0), b"null"), (dict(out=0), b"null")]
    cases += [({k: 0}, b"null") for k in ("natoms", "atoms", "nbonds", "bonds", "priority", "canon_atoms", "canon_bonds", "nodes", "flags")]
    for kw, what in cases:
        assert canon(**kw) == 2, kw
        assert what in lib.mdt_last_error() and b"mdt_mol_canon" in lib.mdt_last_error(), (kw, lib.mdt_last_error())
    assert canon(R_=0) == 0 and canon(R_=0, p=0, out=0) == 0                 # nothing to do: nothing is launched or read
    assert canon(R_=0, L=65) != 0 and canon(R_=0, L=0) != 0


def test_op_schema_and_shape_inference():
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert str(torch.ops.mdt.mol_canon.default._schema) == \
        "mdt::mol_canon(Tensor natoms, Tensor atoms, Tensor nbonds, Tensor bonds) -> (Tensor, Tensor, Tensor, Tensor, Tensor)"
    with FakeTensorMode():
        n, rows = torch.empty(15, dtype=torch.int32), torch.empty(15, 40, dtype=torch.int32)
        out = torch.ops.mdt.mol_canon(n, rows, n, rows)
        assert [(tuple(t.shape), t.dtype) for t in out] == [((15, 40), torch.int64), ((15, 40), torch.int32), ((15, 40), torch.int32),
                                                            ((15,), torch.int32), ((15,), torch.uint8)]
    n, rows = torch.zeros(3, dtype=torch.int32), torch.zeros(3, 4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU implementation"):          # no CPU implementation behind the op
        torch.ops.mdt.mol_canon(n, rows, n, rows)


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


R_, L_ = 7, 16
FORM = ["mdt_mol_hydrogens", "mdt_mol_rings", "mdt_mol_normalize"]
TAIL = ["mdt_mol_rank", "mdt_mol_canon", "mdt_mol_write"]


def names(rec):
    return [e[0] for e in rec.log]


def vocabulary():
    return M.SmilesVocabulary([None] + S.CHARS)


def test_the_op_on_a_recording_library(rec):
    n, rows = torch.zeros(R_, dtype=torch.int32), torch.zeros(R_, L_, dtype=torch.int32)
    out = torch.ops.mdt.mol_canon(n, rows, n, rows)
    assert names(rec) == ["mdt_mol_canon"] and rec.log[0][5:7] == (L_, R_) and rec.log[0][7:12] == tuple(t.data_ptr() for t in out)
    rec.log.clear()
    none, wide = torch.zeros(0, dtype=torch.int32), torch.zeros(0, L_, dtype=torch.int32)
    assert [tuple(t.shape) for t in torch.ops.mdt.mol_canon(none, wide, none, wide)] == [(0, L_)] * 3 + [(0,)] * 2       # R == 0 launches nothing
    too_wide = torch.zeros(R_, 65, dtype=torch.int32)
    for call in (lambda: torch.ops.mdt.mol_canon(n, too_wide, n, too_wide), lambda: torch.ops.mdt.mol_canon(n, rows.long(), n, rows),
                 lambda: torch.ops.mdt.mol_canon(n[:3], rows, n, rows), lambda: torch.ops.mdt.mol_canon(n, rows, n, rows[:, :5])):
        with pytest.raises(RuntimeError, match="mdt::mol_canon"):
            call()
    assert rec.log == []                                                     # refused before any launch


def test_launch_order_of_the_public_calls_with_the_search(rec):
    tok, v = torch.ones(R_, L_, dtype=torch.long), vocabulary()
    head = ["mdt_tokens_compact", "mdt_mol_graph"]
    out = M.mol_respell(tok.to(torch.int16), v, "cpu", canonical=True)
    assert names(rec) == head + TAIL
    graph, rank, canon, write = rec.log[1:5]
    assert rank[1:5] == graph[8:12] == canon[1:5] == write[1:5] and write[5] not in (0, canon[7]) and write[9] == L_
    assert [tuple(t.shape) for t in out] == [(R_, L_), (R_,), (R_,), (R_,)] and all(t.dtype == torch.int64 for t in out)
    rec.log.clear()
    M.mol_respell(tok, v, "cpu", normalize=True, canonical=True, width=128)
    assert names(rec) == head + FORM + TAIL and rec.log[-1][9] == 128
    rec.log.clear()
    M.scaffold_tokens(tok, v, "cpu", generic=True, width=40, canonical=True)
    assert names(rec) == head + ["mdt_mol_scaffold"] + TAIL
    scaf, rank, canon, write = rec.log[2:6]
    assert rank[1:5] == scaf[8:12] == canon[1:5] == write[1:5] and write[9] == 40            # the scaffold arrays are searched and written
    rec.log.clear()
    out = M.scaffold_keep(tok, v, "cpu", canonical=True)
    assert names(rec) == head + ["mdt_mol_scaffold"] + TAIL
    graph, scaf, rank, canon, write = rec.log[1:6]
    assert scaf[1:5] == graph[8:12] == rank[1:5] == canon[1:5] == write[1:5]                  # the MOLECULE is searched and written
    assert [tuple(t.shape) for t in out] == [(R_, L_), (R_, L_), (R_,), (R_,), (R_,)] and out[1].dtype == torch.bool
    rec.log.clear()
    n, rows = torch.ones(R_, dtype=torch.long), torch.ones(R_, L_, dtype=torch.long)
    out = M.mol_write(n, rows, n, rows, v, "cpu", width=30, canonical=True)
    assert names(rec) == TAIL and rec.log[2][9] == 30 and [tuple(t.shape) for t in out] == [(R_, 30), (R_,), (R_, 30), (R_,)]
    rec.log.clear()
    out = M.mol_canon(tok, v, "cpu")
    assert names(rec) == head + ["mdt_mol_canon"] and rec.log[2][1:5] == rec.log[1][8:12]
    assert [tuple(t.shape) for t in out] == [(R_, L_)] * 3 + [(R_,)] * 6 and all(t.dtype == torch.int64 for t in out)
    rec.log.clear()
    M.mol_canon(tok, v, "cpu", normalize=True)
    assert names(rec) == head + FORM + ["mdt_mol_canon"]
    rec.log.clear()
    same, undecided = M.mol_same(tok, torch.ones(R_, 9, dtype=torch.int32), v, "cpu")
    assert names(rec) == (head + ["mdt_mol_canon"]) * 2 and (rec.log[2][5], rec.log[5][5]) == (L_, 9)
    assert same.dtype == undecided.dtype == torch.bool and same.shape == undecided.shape == (R_,)     # (the recorder writes no output: the values are nobody's)
    rec.log.clear()
    for kw in (dict(), dict(canonical=False)):                               # the default: what was launched before the keyword
        M.mol_respell(tok, v, "cpu", **kw), M.scaffold_keep(tok, v, "cpu", **kw), M.mol_write(n, rows, n, rows, v, "cpu", width=8, **kw)
        assert names(rec) == head + ["mdt_mol_rank", "mdt_mol_write"] + head + ["mdt_mol_scaffold", "mdt_mol_rank", "mdt_mol_write"] + \
            ["mdt_mol_rank", "mdt_mol_write"]
        assert rec.log[3][5] == rec.log[2][7]                                # mdt_mol_rank's own tensor goes to the writer
        rec.log.clear()
    empty = torch.zeros(0, L_, dtype=torch.long)                             # no rows: nothing is launched
    assert M.mol_respell(empty, v, "cpu", canonical=True)[0].shape == (0, L_) and M.mol_canon(empty, v, "cpu")[0].shape == (0, L_)
    assert M.mol_same(empty, empty, v, "cpu")[0].shape == (0,) and rec.log == []


def test_the_public_calls_refuse_before_any_launch(rec):
    tok, v = torch.ones(R_, L_, dtype=torch.long), vocabulary()
    n, rows = torch.ones(R_, dtype=torch.long), torch.ones(R_, L_, dtype=torch.long)
    bad = [lambda: M.mol_respell(tok, v, "cpu", canonical=True, invariant=False), lambda: M.mol_respell(tok, v, "cpu", canonical=1),
           lambda: M.mol_write(n, rows, n, rows, v, "cpu", width=8, canonical=True, invariant=False),
           lambda: M.mol_write(n, rows, n, rows, v, "cpu", width=8, canonical=None), lambda: M.scaffold_tokens(tok, v, "cpu", canonical="yes"),
           lambda: M.scaffold_keep(tok, v, "cpu", canonical=0), lambda: M.mol_canon(tok, v, "cpu", normalize=None),
           lambda: M.mol_canon(torch.ones(R_, 65, dtype=torch.long), v, "cpu"), lambda: M.mol_canon(tok.float(), v, "cpu"),
           lambda: M.mol_canon(tok, None, "cpu"), lambda: M.mol_same(tok, tok[:3], v, "cpu"), lambda: M.mol_same(tok, tok, "CNO", "cpu"),
           lambda: M.mol_same(tok, torch.ones(R_, 65, dtype=torch.long), v, "cpu"), lambda: M.mol_same(tok, tok, v, "cpu", normalize=1)]
    for call in bad:
        with pytest.raises(ValueError):
            call()
    assert rec.log == []
