"""No GPU: the definition of the scaffold of a graph row (include/mdt_hip.h, mdt_mol_scaffold) on its reference
(tests/molscaf_ref.py) -- the core against networkx's 2-core and against molring_ref's rings, the exocyclic atoms, the table written
by hand, spellings that share a scaffold, idempotence, GENERIC, the H clamp, the longest peels -- the selection rule of
mdt_screen_select_classes restated in Python, and the plumbing: C exports and argument checks, op schemas and shape inference, the
refusals, and the launch order of the public calls and of the screening call with the scaffold keywords on a recording library."""
import contextlib
import inspect
import os
import re

import numpy as np
import pytest
import torch

import molkey_ref as K
import molnorm_ref as N
import molring_ref as R
import molscaf_ref as C
import screen_ref as SR
import smiles_ref as S
from conftest import ROOT
import moleculediffusiontransformer_amd as M
from moleculediffusiontransformer_amd import generative as G, ops, runtime as rt


@pytest.fixture(scope="module")
def spelled():
    return K.random_spellings()


@pytest.fixture(scope="module")
def pool(spelled):
    return [s for _, sp in spelled for s in sp] + [s[:64] for s in S.mutated_rows(128)] + list(N.TABLE)


def molecules(pool):
    return [s for s in pool if C.string_scaffold(s, 1)["flags"] & C.MOLECULE]


# ---------------------------------------------------------------------------------------------------------------------
# the definition on the reference
# ---------------------------------------------------------------------------------------------------------------------
def test_the_pool_holds_what_the_comparisons_need(pool):
    rows = molecules(pool)
    out = [C.string_scaffold(s, 1) for s in rows]
    scaffold = sum(1 for r in out if r["flags"] & C.SCAFFOLD)
    pruned = sum(1 for r in out if r["flags"] & C.SCAFFOLD and not r["flags"] & C.WHOLE)
    exo = sum(1 for r in out if r["exo"])
    rounds = max(r["rounds"] for r in out)
    print("molecule rows: %d, with a scaffold: %d, pruned: %d, with an exocyclic atom: %d, most rounds: %d" % (len(rows), scaffold, pruned, exo, rounds))
    assert scaffold >= 1000 and pruned >= 800 and exo >= 100


def test_the_core_is_networkx_2_core_and_agrees_with_the_ring_reference(pool):
    import networkx as nx
    asked = 0
    for s in molecules(pool):
        n, atoms, nb, bonds = C.input_arrays(s)
        out = C.string_scaffold(s, 1)
        g = nx.Graph()
        g.add_nodes_from(range(n))
        g.add_edges_from((a, b) for a, b, _ in bonds if a != b)
        assert out["core"] == set(nx.k_core(g, 2).nodes), s
        adj = R.ring_graph(n, bonds)
        for x in out["exo"]:                                                 # exactly one neighbour in the core, none in X
            assert x not in out["core"] and len(adj[x] & out["core"]) == 1 and not adj[x] & out["exo"], s
        rings = R.string_rings(s)
        assert (not out["core"]) == (rings["desc"][5] == 0), s
        assert {x for x in range(n) if rings["atom_ring"][x] > 0} <= out["core"], s
        assert C.string_scaffold(s, 0)["core"] == out["core"] and not C.string_scaffold(s, 0)["exo"]
        assert out["rounds"] <= max(1, n - 1)
        asked += 1
    assert asked >= 2000


def test_words_counts_map_and_flags_of_every_row_in_every_mode(pool):
    for s in pool:
        n, atoms, nb, bonds = C.input_arrays(s)
        for mode in C.MODES:
            r = C.string_scaffold(s, mode)
            if not r["flags"]:
                assert not any(r["atoms"] + r["bonds"] + r["atom_map"]) and r["n"] == r["nb"] == 0 and n == 0, s
                continue
            kept = sorted(r["core"] | r["exo"])
            assert r["n"] == len(kept) and r["flags"] == 1 | 2 * bool(kept) | 4 * (len(kept) == n), (s, mode)
            assert [x for x in range(n) if r["atom_map"][x]] == kept and [r["atom_map"][x] for x in kept] == list(range(1, len(kept) + 1))
            assert not any(r["atoms"][r["n"]:] + r["bonds"][r["nb"]:] + r["atom_map"][n:])
            want = [(r["atom_map"][a] - 1, r["atom_map"][b] - 1, 1 if mode & 2 else o) for a, b, o in bonds
                    if a != b and r["atom_map"][a] and r["atom_map"][b]]
            assert C.unpacked(r)[1] == want, (s, mode)
            if mode & 2:
                assert set(r["atoms"][:r["n"]]) <= {C.PLAIN_C}
            else:
                for x in kept:
                    d, was = r["atoms"][r["atom_map"][x] - 1], atoms[x]
                    lost = sum(C.weight(o) for a, b, o in bonds if a != b and x in (a, b) and not r["atom_map"][a + b - x])
                    assert d == (was if not was >> 11 & 1 else (was & ~(15 << 17)) | min(15, (was >> 17 & 15) + lost) << 17), (s, mode)
            if not mode & 1:
                assert not r["exo"]


@pytest.mark.parametrize("s", list(C.TABLE))
def test_the_hand_table(s):
    for mode, scaffold in zip((1, 0), C.TABLE[s]):
        out = C.string_scaffold(s, mode)
        assert out["flags"] & C.MOLECULE and bool(out["flags"] & C.SCAFFOLD) == (scaffold is not None)
        if scaffold is None:
            assert C.scaffold_key(s, mode) == 0 == C.scaffold_key(s, mode, True) and not any(out["atoms"] + out["bonds"] + out["atom_map"])
            continue
        assert C.scaffold_key(s, mode) == K.string_key(scaffold) != 0, (s, mode)
        assert C.scaffold_key(s, mode, True) == N.normal_key(scaffold) != 0, (s, mode)
        whole = C.string_scaffold(scaffold, mode)                            # the scaffold's own spelling is its own scaffold
        assert whole["flags"] == 7 and C.key_of(whole) == K.string_key(scaffold)


def test_what_the_table_and_its_neighbours_say():
    for s in ("Cc1ccccc1", "CC(=O)c1ccccc1", "O=C(c1ccccc1)c1ccccc1", "O=C1CCCCC1", "CC(C)c1ccc(CC2CC2)cc1", "C1CC1.CCO", "C12CC12", "CCO"):
        assert s in C.TABLE, s
    assert C.scaffold_key("Cn1cccc1", 1, True) == N.normal_key("[nH]1cccc1") != 0       # the H rule on the normal form
    assert C.scaffold_key("Cn1cccc1", 1) == K.string_key("n1cccc1") != K.string_key("[nH]1cccc1")   # as written: implicit, untouched
    assert C.scaffold_key("Cc1ccccc1", 1) != C.scaffold_key("CC1=CC=CC=C1", 1)           # as written two spellings,
    assert C.scaffold_key("Cc1ccccc1", 1, True) == C.scaffold_key("CC1=CC=CC=C1", 1, True) == N.normal_key("c1ccccc1")   # normalised one
    toluene = C.string_scaffold("Cc1ccccc1", 1, True)
    assert toluene["atoms"][0] >> 17 & 15 == 1 and toluene["atoms"][0] >> 10 & 3 == 3 and toluene["atom_map"][:7] == [0, 1, 2, 3, 4, 5, 6]
    ketone = C.string_scaffold("O=C1CCCCC1", 0, True)                        # the bit clear: the ring C loses =O and gains two H
    assert ketone["atoms"][0] >> 17 & 15 == 2 and ketone["n"] == 6 and C.string_scaffold("O=C1CCCCC1", 1, True)["n"] == 7
    both = C.string_scaffold("C1CC1.CCO", 1)                                 # over all components
    assert both["atom_map"][:6] == [1, 2, 3, 0, 0, 0] and both["flags"] == 3
    two = C.string_scaffold("C1CC1.C1CCC1CC", 1)
    assert two["n"] == 7 and two["nb"] == 7 and two["core"] == set(range(7))
    link = C.string_scaffold("CC(C)c1ccc(CC2CC2)cc1", 1)                      # the linker CH2 stays, the isopropyl goes
    assert link["n"] == 10 and link["atom_map"][:3] == [0, 0, 0] and link["atom_map"][7] == 5
    assert C.scaffold_key("CC(=O)c1ccccc1", 1) == C.scaffold_key("Cc1ccccc1", 1)         # =O on a side chain is no exocyclic atom
    assert C.scaffold_key("O=C1CCCCC1", 1) != C.scaffold_key("O=C1CCCCC1", 0) == K.string_key("C1CCCCC1")
    assert C.scaffold_key("O=C1CCCCC1", 3) == K.string_key("CC1CCCCC1") and C.scaffold_key("c1ccncc1", 2) == K.string_key("C1CCCCC1")


def test_the_four_spellings_of_every_graph_share_a_scaffold_key_in_every_mode(spelled):
    with_scaffold = 0
    for _, sp in spelled:
        for mode in C.MODES:
            assert len({C.scaffold_key(s, mode) for s in sp}) == 1, (sp, mode)
            assert len({C.string_scaffold(s, mode)["flags"] for s in sp}) == 1, (sp, mode)
        assert len({C.scaffold_key(s, 1, True) for s in sp}) == 1, sp
        with_scaffold += bool(C.scaffold_key(sp[0], 1))
    assert len(spelled) == 500 and with_scaffold > 250


def test_applying_it_again_is_the_identity_in_modes_0_1_2_and_not_in_mode_3(pool):
    asked = dropped = 0
    for s in pool:
        for normalize in (False, True):
            for mode in (0, 1, 2):
                r = C.string_scaffold(s, mode, normalize)
                if not r["flags"] & C.SCAFFOLD:
                    continue
                twice = C.again(r, mode)
                assert (twice["n"], twice["nb"], twice["atoms"], twice["bonds"], twice["flags"]) == (r["n"], r["nb"], r["atoms"], r["bonds"], 7), (s, mode)
                assert twice["atom_map"][:r["n"]] == list(range(1, r["n"] + 1))
                asked += 1
            r = C.string_scaffold(s, 3, normalize)
            if r["exo"]:                                                     # GENERIC rewrote the exocyclic order: the second pass drops X
                twice = C.again(r, 3)
                assert twice["n"] == r["n"] - len(r["exo"]) == len(r["core"]), s
                dropped += 1
    assert asked > 6000 and dropped > 200


def test_generic_words_the_h_clamp_and_arrays_no_scan_writes():
    special = [C.scaffold_arrays(n, atoms, nb, bonds, mode, width) for width, n, nb, atoms, bonds in C.special_rows() for mode in C.MODES]
    at = lambda row, mode: special[4 * row + mode]  # noqa: E731
    assert at(0, 1)["n"] == 63 and at(0, 0)["n"] == 62 and at(0, 1)["atom_map"][62:64] == [63, 0] and at(0, 1)["nb"] == 63
    assert at(1, 0)["flags"] == 7 and at(1, 0)["n"] == 64 and at(1, 0)["atom_map"] == list(range(1, 65)) and at(1, 0)["rounds"] == 0
    assert at(2, 1)["n"] == 5 and at(2, 1)["nb"] == 6 and at(2, 0)["nb"] == 5 and at(2, 1)["atom_map"][:6] == [1, 2, 3, 4, 5, 0]   # (0, 0) dropped
    # 9 + 4 + 3 clamps at 15; 9 + 2 + 2; 9 + 1 (atoms 6 and 7 close a ring with atom 2 through an entry of order 65535)
    assert [d >> 17 & 15 for d in at(3, 0)["atoms"][:3]] == [15, 13, 10] and [d >> 17 & 15 for d in at(3, 1)["atoms"][:3]] == [15, 9, 10]
    assert at(3, 0)["n"] == 5 and at(3, 1)["n"] == 6 and at(3, 1)["nb"] == 8 and at(3, 1)["bonds"][7] >> 16 == 65535
    assert at(3, 3)["atoms"][:6] == [C.PLAIN_C] * 6 and {w >> 16 for w in at(3, 3)["bonds"][:8]} == {1} and at(3, 3)["n"] == 6
    assert [d >> 17 & 15 for d in at(4, 0)["atoms"][:3]] == [2, 0, 3] and at(4, 0)["atoms"][1] == K.descriptor("C")    # orders 0, 7, 5 weigh 1
    assert at(5, 1)["flags"] == 7 and at(5, 1)["n"] == 4
    for row in range(6, 12):
        assert all(at(row, mode)["flags"] == 0 and not any(at(row, mode)["atoms"] + at(row, mode)["atom_map"]) for mode in C.MODES), row
    assert at(12, 0)["flags"] == 7 and at(12, 0)["nb"] == 28
    assert at(13, 1)["flags"] == 1 and at(13, 1)["n"] == 0 and at(14, 1)["flags"] == 1 and at(14, 1)["rounds"] == 1
    assert C.PLAIN_C == 2 | 9 << 12


def test_the_longest_peels():
    chain = C.string_scaffold("C" * 64, 1)
    assert chain["flags"] == 1 and chain["rounds"] == 32 and chain["n"] == 0 and not any(chain["atoms"] + chain["bonds"] + chain["atom_map"])
    tail = "C1CC1" + "C" * 59                                                # 64 tokens: a 3-ring with a tail of 59, one atom a round
    out = C.string_scaffold(tail, 1)
    assert len(tail) == 64 and out["natoms"] == 62 and out["rounds"] == 59 and out["n"] == 3 and out["nb"] == 3 and out["flags"] == 3
    assert out["atom_map"][:4] == [1, 2, 3, 0] and C.key_of(out) == K.string_key("C1CC1")
    ends = C.string_scaffold("C1CC1" + "C" * 54 + "C1CC1", 0)               # a 54-atom linker between two rings stays
    assert ends["flags"] == 7 and ends["rounds"] == 0


def test_the_selection_rule_in_python():
    rng = np.random.default_rng(3)
    N_, G_, K_ = 8, 3, 4
    packed = np.zeros((N_ * G_, 6), np.int32)
    packed[:, 0] = np.arange(1, N_ * G_ + 1)                                 # distinct rows of length 1
    length = np.ones(N_ * G_, np.int32)
    score = rng.random(N_ * G_).astype(np.float32)
    classes = [int(k) for k in rng.integers(0, 3, N_ * G_)]                  # 0: no class; 1, 2
    plain = SR.select(score, packed, length, N_, G_, K_)
    none = C.select_classes(score, packed, length, N_, G_, K_, [0] * (N_ * G_), 1)      # class 0 is never counted
    assert none[0] == plain[0].tolist() and none[1] == plain[1].tolist() and none[2] == plain[2].tolist()
    for m in (1, 2):
        status, index, count = C.select_classes(score, packed, length, N_, G_, K_, classes, m)
        for g in range(G_):
            kept = [c for c in index[g] if c >= 0]
            assert len(kept) == count[g]
            for k in (1, 2):
                assert sum(classes[c * G_ + g] == k for c in kept) <= m
            order = sorted(range(N_), key=lambda c: (score[c * G_ + g], c))
            seen = {0: 0, 1: 0, 2: 0}
            for c in order:                                                  # the rule, once more in order
                k = classes[c * G_ + g]
                if k and seen[k] >= m:
                    assert status[c * G_ + g] == 16 and c not in kept
                elif sum(seen.values()) < K_:
                    assert c in kept and status[c * G_ + g] == 0
                    seen[k] += 1
    status, _, _ = C.select_classes(score, packed, length, N_, G_, K_, [7] * (N_ * G_), 1, reject=[32] + [0] * (N_ * G_ - 1))
    assert status[0] == 32 and sorted(status[g::G_].count(16) for g in range(G_)) == [N_ - 2, N_ - 1, N_ - 1]


# ---------------------------------------------------------------------------------------------------------------------
# header, library, binding
# ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_the_library_exports_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "mdt_hip.h")).read()
    lib = rt.load_library()
    for name, arity in (("mdt_mol_scaffold", 14), ("mdt_screen_select_classes", 25)):
        assert re.search(r"\bint %s\s*\(" % name, hdr) and name in rt.SYMBOLS and hasattr(lib, name)
        assert len(rt.SYMBOLS[name][1]) == arity
    assert int(re.search(r"#define MDT_ABI_VERSION (\d+)", hdr).group(1)) == rt.ABI_VERSION == 5 == lib.mdt_abi_version()
    for name, value in (("EXOCYCLIC", C.EXOCYCLIC), ("GENERIC", C.GENERIC), ("MOLECULE", C.MOLECULE), ("SCAFFOLD", C.SCAFFOLD),
                        ("WHOLE", C.WHOLE)):
        assert int(re.search(r"\bMDT_MOLS_%s = (\d+)" % name, hdr).group(1)) == value == getattr(rt, "MOLS_" + name)
    flat = " ".join(hdr.replace(" * ", " ").split())
    for phrase in ("Not RDKit's MurckoScaffold", "Aromaticity and hydrogens are as handed in", "Stereo is ignored",
                   "An acyclic molecule has NO scaffold", "Such an x has exactly one neighbour in S and none in X, or it would be in the core",
                   "loses its O and gains two H when bracketed", "can leave an aromatic atom with an odd H count",
                   "is the identity, bit for bit, in modes 0, 1 and 2", "GENERIC rewrites the exocyclic order, so a second pass drops X",
                   "it is not promised in general", "there is no step cap", "Class 0 (\"no scaffold\") is never counted",
                   "the 2-core of the ring graph", "an entry listed twice counts twice"):
        assert phrase in flat, phrase
    assert "k_molscaf.hip" in [s for s, _ in __import__("moleculediffusiontransformer_amd.build", fromlist=["SOURCES"]).SOURCES]
    src = open(os.path.join(ROOT, "moleculediffusiontransformer_amd", "csrc", "k_molscaf.hip")).read()
    for used in ("mols_atom_word(", "mols_bond_word(", "mol_index(", "mols_flags(", "mol_graph_ok_wave(", "mdt_molscaf.h", "mdt_finish(", "__ballot("):
        assert used in src, used
    assert "__shared__" not in src and "__syncthreads" not in src            # no LDS, no barrier
    shared = open(os.path.join(ROOT, "moleculediffusiontransformer_amd", "csrc", "mdt_molscaf.h")).read()
    assert "mdt_molnorm.h" in shared and "mdt_molrow.h" in shared                                          # reused, not copied:
    for helper in ("mol_popc", "mol_index", "mol_in", "mol_all"):                                          # the sets are the row header's
        assert helper + "(" in shared and re.search(r"\b(int|bool|uint64_t) " + helper + r"\(", shared) is None, helper
    assert "moln_bond_word(" in shared and "moln_bond_word(int" not in shared and "mols_row(" in shared
    for phrase in ("not RDKit's MurckoScaffold", "Aromaticity and hydrogens are as handed in", "An acyclic molecule has NO scaffold"):
        assert phrase in " ".join(M.mol_scaffold.__doc__.split()), phrase
    readme = " ".join(open(os.path.join(ROOT, "README.md")).read().split())
    assert "mol_scaffold" in readme and "not RDKit's MurckoScaffold" in readme


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = rt.load_library()

    def call(L=32, R_=5, mode=1, p=8, out=8, **one):
        a = dict(natoms=p, atoms=p, nbonds=p, bonds=p, out_natoms=out, out_atoms=out, out_nbonds=out, out_bonds=out, atom_map=out, flags=out)
        a.update(one)
        return lib.mdt_mol_scaffold(a["natoms"], a["atoms"], a["nbonds"], a["bonds"], L, R_, mode, a["out_natoms"], a["out_atoms"],
                                    a["out_nbonds"], a["out_bonds"], a["atom_map"], a["flags"], 0)
    cases = [(dict(L=0), b"L <= 64"), (dict(L=65), b"L <= 64"), (dict(R_=-1), b"R >= 0"), (dict(mode=4), b"mode <= 3"),
             (dict(mode=-1), b"mode <= 3"), (dict(mode=8), b"mode <= 3"), (dict(p=0), b"null"), (dict(out=0), b"null")]
    cases += [({name: 0}, b"null") for name in ("natoms", "atoms", "nbonds", "bonds", "out_natoms", "out_atoms", "out_nbonds", "out_bonds",
                                                "atom_map", "flags")]
    for kw, what in cases:
        assert call(**kw) == 2, kw
        assert what in lib.mdt_last_error(), (kw, lib.mdt_last_error())
    assert call(R_=0) == 0 and call(R_=0, p=0, out=0) == 0                   # nothing to do: nothing is launched or read
    assert call(R_=0, L=65) != 0 and call(R_=0, L=0) != 0 and call(R_=0, mode=4) != 0

    def select(N_=4, G_=2, K_=2, L=8, M_=0, p=8, fp=0, sim=0, classes=8, most=1, out=8):
        return lib.mdt_screen_select_classes(p, p, p, p, L, N_, G_, 0, 0, 0, M_, K_, 0, 1, 1, 0, fp, fp, sim, classes, most, out, out, out, 0)
    for kw, what in ((dict(most=0), b"mdt_screen_select_classes: need max_per_class >= 1"), (dict(most=-3), b"max_per_class >= 1"),
                     (dict(N_=0), b"mdt_screen_select_classes: need 1 <= N"), (dict(K_=5), b"1 <= K <= N"), (dict(L=65), b"1 <= L <= 64"),
                     (dict(M_=-1), b"M >= 0"), (dict(M_=1), b"known-set pointers"), (dict(p=0), b"mdt_screen_select_classes: null pointer"),
                     (dict(out=0), b"null pointer"), (dict(fp=8, sim=0), b"sim_num"), (dict(fp=8, sim=65537), b"sim_num"),
                     (dict(classes=0, p=0), b"mdt_screen_select_diverse: null pointer"),            # NULL classes: forwarded, twice
                     (dict(classes=0, fp=8, sim=1, p=0), b"mdt_screen_select_similar: null pointer")):
        assert select(**kw) == 2, kw
        assert what in lib.mdt_last_error(), (kw, lib.mdt_last_error())
    assert select(G_=0) == 0 and select(G_=0, classes=0, most=0) == 0 and select(G_=0, most=0) == 2


def vocabulary():
    return M.SmilesVocabulary([None] + S.CHARS)


def test_op_schemas_and_shape_inference():
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert str(torch.ops.mdt.mol_scaffold.default._schema) == \
        ("mdt::mol_scaffold(Tensor natoms, Tensor atoms, Tensor nbonds, Tensor bonds, SymInt mode) -> "
         "(Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)")
    schema = str(torch.ops.mdt.screen_select_classes.default._schema)
    assert schema.startswith("mdt::screen_select_classes(Tensor score, Tensor key, Tensor packed, Tensor length, SymInt candidates, SymInt keep, ")
    assert schema.endswith("Tensor? fp, Tensor? fp_count, SymInt sim_num, Tensor? class_key, SymInt max_per_class) -> (Tensor, Tensor, Tensor)")
    with FakeTensorMode():
        n, rows = torch.empty(15, dtype=torch.int32), torch.empty(15, 40, dtype=torch.int32)
        out = torch.ops.mdt.mol_scaffold(n, rows, n, rows, 3)
        assert [(tuple(t.shape), t.dtype) for t in out] == [((15,), torch.int32), ((15, 40), torch.int32), ((15,), torch.int32),
                                                            ((15, 40), torch.int32), ((15, 40), torch.uint8), ((15,), torch.uint8)]
        score, key = torch.empty(12), torch.empty(12, dtype=torch.int64)
        packed, length = torch.empty(12, 9, dtype=torch.int32), torch.empty(12, dtype=torch.int32)
        out = torch.ops.mdt.screen_select_classes(score, key, packed, length, 4, 2, None, None, None, None, 1, 1, None, None, None, 0, key, 1)
        assert [(tuple(t.shape), t.dtype) for t in out] == [((12,), torch.uint8), ((3, 2), torch.int32), ((3,), torch.int32)]
    n, rows = torch.zeros(3, dtype=torch.int32), torch.zeros(3, 4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU implementation"):          # no CPU implementation behind the ops
        torch.ops.mdt.mol_scaffold(n, rows, n, rows, 1)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        torch.ops.mdt.screen_select_classes(torch.zeros(4), torch.zeros(4, dtype=torch.int64), torch.zeros(4, 3, dtype=torch.int32),
                                            torch.zeros(4, dtype=torch.int32), 2, 1, None, None, None, None, 1, 1, None, None, None, 0,
                                            torch.zeros(4, dtype=torch.int64), 1)


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
FORM = ["mdt_mol_hydrogens", "mdt_mol_rings", "mdt_mol_normalize"]


def names(rec):
    return [e[0] for e in rec.log]


def shape_of(rec):
    return [(e[0], len(e), tuple(a for a in e[1:] if isinstance(a, int) and a < 4096)) for e in rec.log]


def test_launch_order_of_the_public_calls(rec):
    tok, v = torch.ones(N_ * G_, L_, dtype=torch.long), vocabulary()
    known = M.KnownSet(torch.ones(4, L_, dtype=torch.long), L_)
    head = ["mdt_tokens_compact", "mdt_mol_graph"]
    for kw, mode in ((dict(), 1), (dict(exocyclic=False), 0), (dict(generic=True), 3), (dict(exocyclic=False, generic=True), 2)):
        rec.log.clear()
        out = M.mol_scaffold(tok.to(torch.int16), v, "cpu", **kw)
        assert names(rec) == head + ["mdt_mol_scaffold"]
        graph, scaf = rec.log[1:3]
        assert scaf[1:5] == graph[8:12] and scaf[5:8] == (L_, N_ * G_, mode) and 0 not in scaf[8:14] and len(set(scaf[8:14])) == 6
        assert [tuple(t.shape) for t in out] == [(N_ * G_,), (N_ * G_, L_), (N_ * G_,), (N_ * G_, L_), (N_ * G_, L_)] + [(N_ * G_,)] * 3
        assert all(t.dtype == torch.int64 for t in out)
        rec.log.clear()
        out = M.scaffold_key(tok, v, "cpu", normalize=True, **kw)
        assert names(rec) == head + FORM + ["mdt_mol_scaffold", "mdt_mol_key"]
        graph, norm, scaf, key = rec.log[1], rec.log[4], rec.log[5], rec.log[6]
        assert (scaf[1], scaf[3]) == (graph[8], graph[10]) and (scaf[2], scaf[4]) == (norm[11], norm[12]) and scaf[7] == mode
        assert key[1:5] == (scaf[8], scaf[9], scaf[10], scaf[11]) and key[5:7] == (L_, N_ * G_)     # the key of the scaffold arrays
        assert [tuple(t.shape) for t in out] == [(N_ * G_,)] * 4 and all(t.dtype == torch.int64 for t in out)
    rec.log.clear()
    M.scaffold_key(tok, v, "cpu")
    assert names(rec) == head + ["mdt_mol_scaffold", "mdt_mol_key"]
    rec.log.clear()                                                          # the known set: cached per argument tuple
    plain = known.scaffold_keys(v, "cpu")
    assert names(rec) == ["mdt_mol_graph", "mdt_mol_scaffold", "mdt_mol_key"] and rec.log[1][7] == 1
    rec.log.clear()
    normal = known.scaffold_keys(v, "cpu", normalize=True)
    assert names(rec) == ["mdt_mol_graph"] + FORM + ["mdt_mol_scaffold", "mdt_mol_key"]
    rec.log.clear()
    bare = known.scaffold_keys(v, "cpu", exocyclic=False, generic=True)
    assert names(rec) == ["mdt_mol_graph", "mdt_mol_scaffold", "mdt_mol_key"] and rec.log[1][7] == 2
    rec.log.clear()
    assert known.scaffold_keys(v, "cpu") is plain and known.scaffold_keys(v, "cpu", normalize=False, exocyclic=True, generic=False) is plain
    assert known.scaffold_keys(v, "cpu", normalize=True) is normal and known.scaffold_keys(v, "cpu", exocyclic=False, generic=True) is bare
    assert rec.log == [] and plain.dtype == torch.int64 and known.mol_keys(v, "cpu") is not plain


def test_launch_order_of_the_screening_call_with_the_scaffold_keywords(rec):
    tok, cond, v = torch.ones(N_ * G_, L_, dtype=torch.long), torch.zeros(G_, n_), vocabulary()
    known = M.KnownSet(torch.ones(4, L_, dtype=torch.long), L_)
    bad = M.SubstructureSet(["C#N", "OO"], v)
    bad.on("cpu")
    limits = M.DescriptorLimits.lipinski()
    run = lambda **kw: (rec.log.clear(), M.screen_tokens_diverse(Fwd(rec), tok, cond, "cpu", N_, K_, **kw), names(rec)[3:])[2]  # noqa: E731
    today = [
        (dict(), ["mdt_screen_select"]),
        (dict(vocabulary=v), ["mdt_smiles_check", "mdt_screen_select_reject"]),
        (dict(known_tokens=known, min_novelty=2), ["mdt_edit_nearest", "mdt_screen_select_diverse"]),
        (dict(vocabulary=v, identity="graph", known_tokens=known), ["mdt_smiles_check", "mdt_mol_graph", "mdt_mol_key", "mdt_key_flags", "mdt_screen_select_reject"]),
        (dict(vocabulary=v, max_similarity=0.5), ["mdt_smiles_check", "mdt_mol_graph", "mdt_mol_fp", "mdt_screen_select_similar"]),
        (dict(vocabulary=v, identity="graph", limits=limits, forbid=bad, normalize=True),
         ["mdt_smiles_check", "mdt_mol_graph"] + FORM + ["mdt_mol_key", "mdt_key_flags", "mdt_sub_match", "mdt_screen_select_reject"]),
        (dict(vocabulary=v, known_tokens=known, max_known_similarity=0.7, min_distance=3),
         ["mdt_smiles_check", "mdt_mol_graph", "mdt_mol_fp", "mdt_fp_nearest", "mdt_screen_select_diverse_reject"])]
    for normal in (False, True):                                             # (the known set's keys and fingerprints: once)
        known.mol_keys(v, "cpu", normalize=normal), known.fingerprints(v, "cpu", normalize=normal), known.scaffold_keys(v, "cpu", normalize=normal)
        known.scaffold_keys(v, "cpu", normalize=normal, exocyclic=False, generic=True)
    asked, keys_of = [], known.scaffold_keys
    known.scaffold_keys = lambda *a, **k: asked.append(k) or keys_of(*a, **k)
    for kw, want in today:
        logs = []
        for extra in (dict(), dict(max_per_scaffold=None, novel_scaffold=False, scaffold_exocyclic=True, scaffold_generic=False),
                      dict(scaffold_exocyclic=False, scaffold_generic=True)):    # the defaults: today's log, argument for argument
            assert run(**kw, **extra) == want, kw
            logs.append(shape_of(rec))
        assert logs[0] == logs[1] == logs[2] and asked == []
        if "vocabulary" not in kw:
            continue
        base = [w for w in want[:-1]]
        if "mdt_mol_graph" not in base:
            base.append("mdt_mol_graph")
        # max_per_scaffold: one mol_scaffold and one mol_key after everything that reads the graph, then the class selection
        got = run(**kw, max_per_scaffold=2)
        assert got == base + ["mdt_mol_scaffold", "mdt_mol_key", "mdt_screen_select_classes"], kw
        assert got.count("mdt_mol_graph") == 1 and asked == []
        at = {name: rec.log[3 + len(got) - 1 - got[::-1].index(name)] for name in got}        # (the last launch of each name)
        graph, scaf, key, sel = at["mdt_mol_graph"], at["mdt_mol_scaffold"], at["mdt_mol_key"], at["mdt_screen_select_classes"]
        assert (scaf[1], scaf[3]) == (graph[8], graph[10]) and scaf[5:8] == (L_, N_ * G_, 1) and key[1:5] == scaf[8:12]
        if kw.get("normalize"):
            norm = at["mdt_mol_normalize"]
            assert (scaf[2], scaf[4]) == (norm[11], norm[12])                # the scaffold of the normal form
        else:
            assert (scaf[2], scaf[4]) == (graph[9], graph[11])
        assert len(sel) == 26 and sel[20] == key[7] != 0 and sel[21] == 2 and sel[5:8] == (L_, N_, G_) and sel[16] != 0
        assert sel[14:16] == (1, kw.get("min_distance", 1))
        with_fp = "max_similarity" in kw
        assert (sel[17] != 0) == (sel[18] != 0) == with_fp and sel[19] == (32768 if with_fp else 0)
        # novel_scaffold alone: the known set's scaffold keys through key_flags, today's selection
        got = run(**{**kw, "known_tokens": known}, novel_scaffold=True, scaffold_exocyclic=False, scaffold_generic=True)
        assert got[-4:] == ["mdt_mol_scaffold", "mdt_mol_key", "mdt_key_flags", want[-1]], kw
        assert got.count("mdt_mol_graph") == 1 and rec.log[-4][7] == 2
        assert asked == [dict(normalize=bool(kw.get("normalize")), exocyclic=False, generic=True)]
        assert rec.log[-2][1] == rec.log[-3][7] != 0 and rec.log[-2][2:4] == (N_, G_)    # key_flags reads the scaffold keys
        del asked[:]
        got = run(**{**kw, "known_tokens": known}, novel_scaffold=True, max_per_scaffold=1)
        assert got[-4:] == ["mdt_mol_scaffold", "mdt_mol_key", "mdt_key_flags", "mdt_screen_select_classes"] and got.count("mdt_mol_scaffold") == 1
        del asked[:]
    assert run(vocabulary=v, normalize=True, max_per_scaffold=1) == \
        ["mdt_smiles_check", "mdt_mol_graph"] + FORM + ["mdt_mol_scaffold", "mdt_mol_key", "mdt_screen_select_classes"]       # a consumer of normalize


def test_screen_candidates_forwards_the_scaffold_keywords_only_when_set(rec, monkeypatch):
    seen = {}

    class Inv:
        max_length = 32

        def sample_tokens(self, seq, device, **k):
            return torch.ones(seq.shape[0], 32, dtype=torch.long)
    monkeypatch.setattr(G, "screen_tokens", lambda *a, **k: seen.update(plain=k) or "plain")
    monkeypatch.setattr(G, "screen_tokens_diverse", lambda *a, **k: seen.update(diverse=k) or "diverse")
    cond, v = torch.zeros(2, 12), vocabulary()
    known = M.KnownSet(torch.ones(4, 32, dtype=torch.long), 32)
    assert M.screen_candidates(Inv(), "fwd", cond, "dev", 3, 2, vocabulary=v, max_per_scaffold=1, scaffold_generic=True) == "diverse"
    assert seen["diverse"] == dict(min_distance=1, min_novelty=1, vocabulary=v, max_per_scaffold=1, scaffold_generic=True)
    assert M.screen_candidates(Inv(), "fwd", cond, "dev", 3, 2, vocabulary=v, known_tokens=known, novel_scaffold=True, normalize=True) == "diverse"
    assert seen["diverse"] == dict(min_distance=1, min_novelty=1, vocabulary=v, novel_scaffold=True, normalize=True, known_tokens=known)
    assert M.screen_candidates(Inv(), "fwd", cond, "dev", 3, 2, max_per_scaffold=None, novel_scaffold=False, scaffold_exocyclic=False) == "plain"
    assert seen["plain"] == dict() and rec.log == []


def test_refusals_come_before_anything_is_launched(rec):
    fwd, v = Fwd(rec), vocabulary()
    tok, cond = torch.ones(N_ * G_, L_, dtype=torch.long), torch.zeros(G_, n_)
    wide = torch.ones(N_ * G_, 65, dtype=torch.long)
    known = M.KnownSet(torch.ones(4, L_, dtype=torch.long), L_)
    empty = M.KnownSet(torch.zeros(0, L_, dtype=torch.long), L_)
    div = lambda t=tok, **kw: M.screen_tokens_diverse(fwd, t, cond, "cpu", N_, K_, **kw)  # noqa: E731

    class Inv:
        max_length = 65

        def sample_tokens(self, *a, **k):
            raise AssertionError("sampled")

    class Inv32(Inv):
        max_length = 32
    for call, what in (
            (lambda: div(max_per_scaffold=1), "give a vocabulary"),
            (lambda: div(novel_scaffold=True, known_tokens=known), "give a vocabulary"),
            (lambda: div(wide, vocabulary=v, max_per_scaffold=1), "at most 64"),
            (lambda: div(vocabulary=v, max_per_scaffold=0), "int >= 1 or None"),
            (lambda: div(vocabulary=v, max_per_scaffold=True), "int >= 1 or None"),
            (lambda: div(vocabulary=v, max_per_scaffold=1.0), "int >= 1 or None"),
            (lambda: div(vocabulary=v, novel_scaffold=1, known_tokens=known), "novel_scaffold must be True or False"),
            (lambda: div(vocabulary=v, novel_scaffold=True), "non-empty known_tokens"),
            (lambda: div(vocabulary=v, novel_scaffold=True, known_tokens=empty), "non-empty known_tokens"),
            (lambda: div(vocabulary=v, max_per_scaffold=1, scaffold_exocyclic=1), "scaffold_exocyclic must be True or False"),
            (lambda: div(vocabulary=v, scaffold_generic=None), "scaffold_generic must be True or False"),
            (lambda: div(vocabulary=v, normalize=True), "ask for one of them"),
            (lambda: M.screen_candidates(Inv(), fwd, cond, "cpu", N_, K_, vocabulary=v, max_per_scaffold=1), "at most 64"),
            (lambda: M.screen_candidates(Inv32(), fwd, cond, "cpu", N_, K_, max_per_scaffold=1), "give a vocabulary"),
            (lambda: M.screen_candidates(Inv32(), fwd, cond, "cpu", N_, K_, vocabulary=v, novel_scaffold=True), "non-empty known_tokens"),
            (lambda: M.screen_candidates(Inv32(), fwd, cond, "cpu", N_, K_, vocabulary=v, max_per_scaffold=-1), "int >= 1 or None"),
            (lambda: M.mol_scaffold(wide, v, "cpu"), "at most 64"),
            (lambda: M.mol_scaffold(tok.float(), v, "cpu"), "integer"),
            (lambda: M.mol_scaffold(tok, S.CHARS, "cpu"), "SmilesVocabulary"),
            (lambda: M.mol_scaffold(tok[:, :0], v, "cpu"), "at least one position"),
            (lambda: M.mol_scaffold(tok, v, "cpu", normalize=1), "normalize must be True or False"),
            (lambda: M.mol_scaffold(tok, v, "cpu", exocyclic=1), "exocyclic must be True or False"),
            (lambda: M.scaffold_key(tok, v, "cpu", generic="no"), "generic must be True or False"),
            (lambda: M.scaffold_key(wide, v, "cpu"), "at most 64"),
            (lambda: known.scaffold_keys(v, "cpu", normalize=1), "True or False"),
            (lambda: known.scaffold_keys(v, "cpu", generic=0), "True or False"),
            (lambda: known.scaffold_keys(S.CHARS, "cpu"), "SmilesVocabulary"),
            (lambda: M.KnownSet(torch.ones(2, 65, dtype=torch.long), 65).scaffold_keys(v, "cpu"), "at most 64")):
        with pytest.raises(ValueError, match=what):
            call()
    assert rec.log == []
    with pytest.raises(TypeError):                                           # screen_tokens keeps its parameter list
        M.screen_tokens(fwd, tok, cond, "cpu", N_, K_, max_per_scaffold=1)
    with pytest.raises(TypeError):                                           # keyword-only
        M.mol_scaffold(tok, v, "cpu", True)
    n, rows = torch.zeros(3, dtype=torch.int32), torch.zeros(3, 8, dtype=torch.int32)
    scaf, w65 = torch.ops.mdt.mol_scaffold, torch.zeros(3, 65, dtype=torch.int32)
    score, key, packed, length = torch.zeros(6), torch.zeros(6, dtype=torch.int64), torch.zeros(6, 8, dtype=torch.int32), torch.zeros(6, dtype=torch.int32)
    sel = lambda class_key=key, most=1, p=packed: torch.ops.mdt.screen_select_classes(  # noqa: E731
        score, key, p, length, 3, 2, None, None, None, None, 1, 1, None, None, None, 0, class_key, most)
    for call, what in ((lambda: scaf(n, w65, n, w65, 1), "1 to 64"), (lambda: scaf(n, rows[:, :0], n, rows[:, :0], 1), "1 to 64"),
                       (lambda: scaf(n, rows.long(), n, rows, 1), "int32"), (lambda: scaf(n[:2], rows, n, rows, 1), "one value per row"),
                       (lambda: scaf(n, rows, n, rows, 4), "mode = 4"), (lambda: scaf(n, rows, n, rows, -1), "mode = -1"),
                       (lambda: sel(most=0), "max_per_class = 0"), (lambda: sel(class_key=key.int()), "class_key must hold one int64"),
                       (lambda: sel(class_key=key[:5]), "class_key must hold one int64"),
                       (lambda: sel(p=torch.zeros(6, 65, dtype=torch.int32)), "exceed the 64")):
        with pytest.raises(RuntimeError, match=what):
            call()
    assert rec.log == []


def test_public_surface():
    for name in ("mol_scaffold", "scaffold_key"):
        assert getattr(M, name) is getattr(G, name)
        p = inspect.signature(getattr(M, name)).parameters
        assert list(p) == ["tokens", "vocabulary", "device", "normalize", "exocyclic", "generic"]
        assert [p[k].default for k in ("normalize", "exocyclic", "generic")] == [False, True, False]
        assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("normalize", "exocyclic", "generic"))
    p = inspect.signature(M.KnownSet.scaffold_keys).parameters
    assert list(p) == ["self", "vocabulary", "device", "normalize", "exocyclic", "generic"] and p["exocyclic"].default is True
    p = inspect.signature(M.screen_tokens_diverse).parameters
    assert [p[k].default for k in ("max_per_scaffold", "novel_scaffold", "scaffold_exocyclic", "scaffold_generic")] == [None, False, True, False]
    assert list(p)[-2:] == ["normalize", "screen_tokens_kwargs"] and "max_per_scaffold" not in inspect.signature(M.screen_tokens).parameters
    flat = " ".join(M.screen_tokens_diverse.__doc__.split())
    for phrase in ("not RDKit's MurckoScaffold", "mdt::mol_graph is never launched twice", "mdt::screen_select_classes",
                   "Candidates without a scaffold (key 0) are never counted", "KnownSet.scaffold_keys()"):
        assert phrase in flat, phrase
