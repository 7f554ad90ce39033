"""No GPU: the definition of ring perception and the descriptors (include/mdt_hip.h, mdt_mol_rings) on its reference
(tests/molring_ref.py) -- the table written by hand, an independent oracle (networkx: bridges, shortest paths, cycle basis,
components) on every molecule row of the pools, invariance under respelling and under renumbering -- and the plumbing: C export and
argument checks, op schema and shape inference, DescriptorLimits, the refusals, and the launch order of the screening call with
``limits`` on a recording library."""
import contextlib
import inspect
import os
import random
import re

import pytest
import torch

import molh_ref as H
import molkey_ref as K
import molring_ref as R
import smiles_ref as S
from conftest import ROOT
import moleculediffusiontransformer_amd as M
from moleculediffusiontransformer_amd import generative as G, ops, runtime as rt

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


@pytest.fixture(scope="module")
def spelled():
    return K.random_spellings()


def pools(spelled):
    rows = list(R.TABLE) + [s for _, sp in spelled for s in sp]
    assert len(rows) - len(R.TABLE) == 2000
    return rows + [s[:64] for s in S.mutated_rows(512)]


# ---------------------------------------------------------------------------------------------------------------------
# the definition on the reference
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", list(R.TABLE))
def test_the_hand_table(s):
    bond_ring, atom_ring, named = R.TABLE[s]
    r = R.string_rings(s)
    _, _, atoms, bonds = K.graph(s)
    assert r["molecule"] and len(s) <= 64 and len(bonds) == len(bond_ring) and len(atoms) == len(atom_ring)
    assert r["bond_ring"][:len(bonds)] == bond_ring and not any(r["bond_ring"][len(bonds):])
    assert r["atom_ring"][:len(atoms)] == atom_ring and not any(r["atom_ring"][len(atoms):])
    got = dict(zip(R.NAMES, r["desc"]))
    assert {k: got[k] for k in named} == named


def test_what_the_table_must_hold():
    for s in ("C", "CC", "C1CC1", "c1ccccc1", "c1ccc2ccccc2c1", "C1CC12CC2", "C12C3C4C1C5C2C3C45", "C1CC2CCC1C2", "c1ccccc1c1ccccc1",
              "CCCC", "CC#CC", "CC(=O)NC", "C.C", "[Na+].[Cl-]", "C12CC12", "cc", "[nH]1cccc1", "CC(=O)O", "[2H]O[2H]", R.WIDEST_RING):
        assert s in R.TABLE, s
    assert len(R.WIDEST_RING) == 64 and R.TABLE[R.WIDEST_RING][0] == [62] * 62
    assert R.TABLE["c1ccc2ccccc2c1"][0][8] == 6 and K.graph("c1ccc2ccccc2c1")[3][8][:2] == (3, 8)      # the fusion bond
    assert R.TABLE["c1ccccc1c1ccccc1"][0][6] == 0 and K.graph("c1ccccc1c1ccccc1")[3][6] == (5, 6, 5)     # the axis: order 5
    assert K.graph("C12CC12")[3][2:] == [(0, 2, 1), (0, 2, 1)]                                         # parallel entries
    assert len(R.NAMES) == 16 and list(R.MILLI.values()) == [round(1000 * H.WEIGHTS[s]) for s in R.MILLI]


def test_rows_that_are_no_molecule_are_all_zero():
    for s in ["", "C(", "C1CC", "c1ccccc", "Xx"] + [s for s, _ in S.MALFORMED_TABLE + S.OVERVALENT_TABLE]:
        r = R.string_rings(s[:64])
        assert not r["molecule"] and not any(r["bond_ring"] + r["atom_ring"] + r["desc"]), s
        assert R.flag(r["desc"], r["molecule"], [1] * 16, [0] * 16) == 0     # bounds nothing can meet: still flag 0
    c = K.descriptor("C")
    for n, nb, bonds in ((3, 1, [(0, 3, 1)]), (9, 0, []), (2, 9, []), (-1, 0, []), (2, -1, []), (0, 0, [])):
        r = R.rings_arrays(n, [c] * 8, nb, bonds, [0] * 8, width=8)
        assert not any(r["bond_ring"] + r["atom_ring"] + r["desc"])


def test_entries_that_no_scan_writes():
    c = K.descriptor("C")
    named = lambda r: dict(zip(R.NAMES, r["desc"]))  # noqa: E731
    twice = R.rings_arrays(3, [c] * 3, 4, [(0, 1, 1), (1, 0, 1), (1, 2, 1), (2, 0, 1)], [2] * 3, width=8)   # listed twice: one edge
    assert twice["bond_ring"][:4] == [3, 3, 3, 3] and named(twice)["rings"] == 1 and named(twice)["ring_bonds"] == 4
    loop = R.rings_arrays(3, [c] * 3, 3, [(0, 0, 1), (0, 1, 1), (1, 2, 3)], [1, 2, 3], width=8)           # (a, a): never an edge
    assert loop["bond_ring"][:3] == [0, 0, 0] and named(loop)["rings"] == 0 and named(loop)["components"] == 1
    assert named(loop)["sp3_carbons"] == 1 and named(loop)["weight"] == 3 * 12011 + 6 * 1008
    odd = R.rings_arrays(4, [c] * 4, 4, [(0, 1, 0), (1, 2, 65535), (2, 3, 1), (3, 0, 1)], [0] * 4, width=8)   # any order is an edge
    assert odd["bond_ring"][:4] == [4] * 4 and odd["atom_ring"][:4] == [4] * 4 and named(odd)["sp3_carbons"] == 1
    two = R.rings_arrays(2, [c] * 2, 2, [(0, 1, 1)] * 2, [3, 3], width=8)    # parallel entries alone make no ring
    assert two["bond_ring"][:2] == [0, 0] and named(two)["rings"] == 0
    chain = R.rings_arrays(4, [c] * 4, 4, [(0, 1, 1), (1, 2, 1), (1, 2, 1), (2, 3, 1)], [0] * 4, width=8)
    assert named(chain)["rotatable_bonds"] == 2                              # an entry listed twice counts twice


def test_an_independent_oracle_on_every_molecule_row(spelled):
    """networkx on the ring graph: bond_ring == 0 exactly for the bridges; otherwise 1 + the shortest path with the edge removed;
    rings == len(cycle_basis); components == number_connected_components.  No molecule row is left out."""
    import networkx as nx
    asked = ringed = 0
    for s in pools(spelled):
        r = R.string_rings(s)
        if not r["molecule"]:
            continue
        _, _, atoms, bonds = K.graph(s)
        g = nx.Graph()
        g.add_nodes_from(range(len(atoms)))
        g.add_edges_from((a, b) for a, b, _ in bonds if a != b)
        bridges = {frozenset(e) for e in nx.bridges(g)}
        for e, (a, b, _) in enumerate(bonds):
            got = r["bond_ring"][e]
            assert (got == 0) == (a == b or frozenset((a, b)) in bridges), (s, e)
            if got:
                cut = g.copy()
                cut.remove_edge(a, b)
                assert got == 1 + nx.shortest_path_length(cut, a, b), (s, e)
        named = dict(zip(R.NAMES, r["desc"]))
        assert named["rings"] == len(nx.cycle_basis(g)), s
        assert named["components"] == nx.number_connected_components(g), s
        if len(atoms) <= 12:                                                 # the smallest cycle through the atom, from all cycles
            cycles = list(nx.simple_cycles(g))
            for a in range(len(atoms)):
                assert r["atom_ring"][a] == min((len(c) for c in cycles if a in c), default=0), (s, a)
        asked += 1
        ringed += named["rings"] > 0
    print("molecule rows asked: %d, with a ring: %d" % (asked, ringed))
    assert asked >= 2021 + 200 and ringed > 900                              # table, spellings and the valid mutated rows


def test_the_descriptors_do_not_depend_on_the_spelling(spelled):
    asked = 0
    for _, sp in spelled:
        first = R.string_rings(sp[0])
        assert first["molecule"]
        for t in sp[1:]:
            other = R.string_rings(t)
            assert other["desc"] == first["desc"], (sp[0], t)
            assert sorted(other["atom_ring"]) == sorted(first["atom_ring"]) and sorted(other["bond_ring"]) == sorted(first["bond_ring"])
            asked += 1
    assert asked == 1500


def test_ring_sizes_follow_the_atoms_and_bonds_through_a_renumbering(spelled):
    rng = random.Random(11)
    rows = list(R.TABLE) + [sp[0] for _, sp in spelled[:200]]
    for s in rows:
        _, _, atoms, bonds = K.graph(s)
        n, nb = len(atoms), len(bonds)
        hydrogens = H.string_hydrogens(s)["hydrogens"][:n]
        base = R.rings_arrays(n, atoms, nb, bonds, hydrogens)
        to = list(range(n))
        rng.shuffle(to)                                                      # old atom a becomes to[a]
        order = list(range(nb))
        rng.shuffle(order)                                                   # new entry k is old entry order[k], its ends swapped at random
        new_atoms, new_h = [0] * n, [0] * n
        for a in range(n):
            new_atoms[to[a]], new_h[to[a]] = atoms[a], hydrogens[a]
        new_bonds = []
        for e in order:
            a, b, o = bonds[e]
            new_bonds.append((to[b], to[a], o) if rng.random() < 0.5 else (to[a], to[b], o))
        again = R.rings_arrays(n, new_atoms, nb, new_bonds, new_h)
        assert again["desc"] == base["desc"], s
        assert [again["bond_ring"][k] for k in range(nb)] == [base["bond_ring"][order[k]] for k in range(nb)], s
        assert [again["atom_ring"][to[a]] for a in range(n)] == base["atom_ring"][:n], s


# ---------------------------------------------------------------------------------------------------------------------
# header, library, binding
# ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_the_library_exports_the_new_symbol():
    hdr = open(os.path.join(ROOT, "include", "mdt_hip.h")).read()
    lib = rt.load_library()
    assert re.search(r"\bint mdt_mol_rings\s*\(", hdr) and "mdt_mol_rings" in rt.SYMBOLS and hasattr(lib, "mdt_mol_rings")
    assert len(rt.SYMBOLS["mdt_mol_rings"][1]) == 14
    assert int(re.search(r"#define MDT_ABI_VERSION (\d+)", hdr).group(1)) == rt.ABI_VERSION == 5 == lib.mdt_abi_version()
    assert int(re.search(r"#define MDT_MOLR_DESC (\d+)", hdr).group(1)) == rt.MOLR_DESC == len(M.DESCRIPTOR_NAMES) == len(R.NAMES) == 16
    assert M.DESCRIPTOR_NAMES == R.NAMES and rt.SCREEN_SUBSTRUCTURE == R.LIMIT_BIT == 128
    for k, name in enumerate(R.NAMES):                                       # every slot has a named enumerator, in this order
        assert int(re.search(r"\bMDT_MOLR_%s = (\d+)" % name.upper(), hdr).group(1)) == k, name
    flat = " ".join(hdr.replace(" * ", " ").split())
    for phrase in ("Not RDKit's ring info and not an SSSR", "No envelope rings", "No logP", "Aromaticity is as written",
                   "AN ORDER-5 ENTRY IS NEVER ROTATABLE", "naphthalene gives 6, not 10", "a descriptor of mdt_mol_rings lies outside its bounds",
                   " ".join(str(v) for v in R.MILLI.values())):
        assert phrase in flat, phrase
    assert "k_molring.hip" in [s for s, _ in __import__("moleculediffusiontransformer_amd.build", fromlist=["SOURCES"]).SOURCES]
    src = open(os.path.join(ROOT, "moleculediffusiontransformer_amd", "csrc", "k_molring.hip")).read()
    assert "molr_mass(" in src and "molh_slot(" in src and "mol_graph_ok_wave(" in src and "mdt_molring.h" in src and "mdt_finish(" in src
    shared = open(os.path.join(ROOT, "moleculediffusiontransformer_amd", "csrc", "mdt_molring.h")).read()
    assert "mdt_molh.h" in shared and "molh_slot(" in shared and "molh_slot(uint32_t" not in shared   # reused, not copied
    assert "mdt_molrow.h" in shared and "int mol_search(" not in shared and "uint64_t mol_component(" not in shared
    for used in ("mol_search(", "mol_component(", "mol_ring_adj(", "mol_popc("):
        assert used in shared, used


def test_entry_point_refuses_bad_arguments_before_any_launch():
    lib = rt.load_library()

    def call(L=32, R_=5, p=8, out=8, lo=8, hi=8, flags=8):
        return lib.mdt_mol_rings(p, p, p, p, p, L, R_, lo, hi, out, out, out, flags, 0)
    for kw, what in ((dict(L=0), b"L <= 64"), (dict(L=65), b"L <= 64"), (dict(R_=-1), b"R >= 0"), (dict(p=0), b"null"), (dict(out=0), b"null"),
                     (dict(lo=0), b"together"), (dict(hi=0), b"together")):
        assert call(**kw) == 2, kw
        assert what in lib.mdt_last_error(), (kw, lib.mdt_last_error())
    assert call(R_=0) == 0 and call(R_=0, p=0, out=0, lo=0, hi=0, flags=0) == 0     # nothing to do: nothing is launched or read
    assert call(R_=0, L=65) != 0 and call(R_=0, lo=0) != 0


def vocabulary():
    return M.SmilesVocabulary([None] + S.CHARS)


def test_op_schema_and_shape_inference():
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert str(torch.ops.mdt.mol_rings.default._schema) == \
        "mdt::mol_rings(Tensor natoms, Tensor atoms, Tensor nbonds, Tensor bonds, Tensor hydrogens, Tensor? lo, Tensor? hi) -> (Tensor, Tensor, Tensor, Tensor)"
    with FakeTensorMode():
        n, rows, h = torch.empty(15, dtype=torch.int32), torch.empty(15, 40, dtype=torch.int32), torch.empty(15, 40, dtype=torch.uint8)
        out = torch.ops.mdt.mol_rings(n, rows, n, rows, h, None, None)
        assert [(tuple(t.shape), t.dtype) for t in out] == [((15, 40), torch.uint8), ((15, 40), torch.uint8), ((15, 16), torch.int32),
                                                            ((15,), torch.uint8)]
    n, rows, h = torch.zeros(3, dtype=torch.int32), torch.zeros(3, 4, dtype=torch.int32), torch.zeros(3, 4, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU implementation"):          # no CPU implementation behind the op
        torch.ops.mdt.mol_rings(n, rows, n, rows, h, None, None)


# ---------------------------------------------------------------------------------------------------------------------
# DescriptorLimits
# ---------------------------------------------------------------------------------------------------------------------
def test_descriptor_limits_parsing_errors_and_milli_dalton():
    none = M.DescriptorLimits()
    assert none.lo.dtype == none.hi.dtype == torch.int32 and none.lo.tolist() == [INT32_MIN] * 16 and none.hi.tolist() == [INT32_MAX] * 16
    for k, name in enumerate(M.DESCRIPTOR_NAMES):                            # every name takes both keywords
        value = 7.5 if name == "weight" else 7
        low, high = M.DescriptorLimits(**{"min_" + name: value}), M.DescriptorLimits(**{"max_" + name: value})
        stored = 7500 if name == "weight" else 7
        assert low.lo[k] == stored and high.hi[k] == stored
        assert low.hi.tolist() == [INT32_MAX] * 16 and high.lo.tolist() == [INT32_MIN] * 16
        assert sum(v != INT32_MIN for v in low.lo.tolist()) == 1 and sum(v != INT32_MAX for v in high.hi.tolist()) == 1
    lim = M.DescriptorLimits(max_rings=4, min_smallest_ring=5, max_rotatable_bonds=10, max_weight=499.9996, min_weight=180)
    named = lambda t: dict(zip(M.DESCRIPTOR_NAMES, t.tolist()))  # noqa: E731
    assert named(lim.hi)["rings"] == 4 and named(lim.lo)["smallest_ring"] == 5 and named(lim.hi)["rotatable_bonds"] == 10
    assert named(lim.hi)["weight"] == 500000 and named(lim.lo)["weight"] == 180000          # dalton -> the nearest milli-dalton
    assert M.DescriptorLimits(max_weight=46.0694).hi[15] == 46069 and M.DescriptorLimits(max_weight=46.0695001).hi[15] == 46070
    lip = M.DescriptorLimits.lipinski()
    assert named(lip.hi)["weight"] == 500000 and named(lip.hi)["donors"] == 5 and named(lip.hi)["acceptors"] == 10
    assert lip.lo.tolist() == [INT32_MIN] * 16 and sum(v != INT32_MAX for v in lip.hi.tolist()) == 3
    assert "logP" in M.DescriptorLimits.lipinski.__doc__ and "not built" in M.DescriptorLimits.lipinski.__doc__
    lo, hi = lim.on("cpu")
    assert torch.equal(lo, lim.lo) and torch.equal(hi, lim.hi) and lim.on("cpu")[0] is lo          # one copy per device
    for bad in (dict(max_ring=1), dict(rings=1), dict(maximum_rings=1), dict(max_logp=5), dict(min_=1), dict(max_Rings=1)):
        with pytest.raises(ValueError, match="min_<name> / max_<name>"):
            M.DescriptorLimits(**bad)
    for bad in (dict(max_rings=1.0), dict(max_rings=True), dict(min_donors="1"), dict(max_rings=2 ** 31), dict(max_rings=None)):
        with pytest.raises(ValueError, match="must be an int"):
            M.DescriptorLimits(**bad)
    for bad in (dict(max_weight="500"), dict(max_weight=True), dict(max_weight=float("nan")), dict(max_weight=float("inf")),
                dict(min_weight=3.0e6)):
        with pytest.raises(ValueError, match="dalton"):
            M.DescriptorLimits(**bad)
    # the flag of the definition on the reference: Lipinski passes aspirin's atoms and refuses a sugar chain's donors
    lo, hi = lip.lo.tolist(), lip.hi.tolist()
    for s, want in (("CC(=O)Oc1ccccc1C(=O)O", 0), ("OCC(O)C(O)C(O)C(O)C(O)CO", 128), ("C(", 0)):
        r = R.string_rings(s)
        assert R.flag(r["desc"], r["molecule"], lo, hi) == want, s


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


def names(rec):
    return [e[0] for e in rec.log]


def test_launch_order_of_the_screening_call_with_and_without_limits(rec):
    tok, cond, v = torch.ones(N_ * G_, L_, dtype=torch.long), torch.zeros(G_, n_), vocabulary()
    known = M.KnownSet(torch.ones(4, L_, dtype=torch.long), L_)
    need, bad = M.SubstructureSet(["C=O", "N"], v), M.SubstructureSet(["C#N", "OO", "c1ccccc1"], v)
    need.on("cpu"), bad.on("cpu")                                            # (the patterns' graphs: once per device, not here)
    limits = M.DescriptorLimits.lipinski()
    run = lambda **kw: (rec.log.clear(), M.screen_tokens_diverse(Fwd(rec), tok, cond, "cpu", N_, K_, **kw), names(rec)[3:])[2]  # noqa: E731
    # today's launches in today's order, as the tests of the earlier keywords list them ...
    today = [
        (dict(), ["mdt_screen_select"]),
        (dict(vocabulary=v), ["mdt_smiles_check", "mdt_screen_select_reject"]),
        (dict(min_distance=2), ["mdt_screen_select_diverse"]),
        (dict(vocabulary=v, min_distance=2), ["mdt_smiles_check", "mdt_screen_select_diverse_reject"]),
        (dict(known_tokens=known, min_novelty=2), ["mdt_edit_nearest", "mdt_screen_select_diverse"]),
        (dict(vocabulary=v, identity="graph"), ["mdt_smiles_check", "mdt_mol_graph", "mdt_mol_key", "mdt_key_flags", "mdt_screen_select_reject"]),
        (dict(vocabulary=v, max_similarity=0.5), ["mdt_smiles_check", "mdt_mol_graph", "mdt_mol_fp", "mdt_screen_select_similar"]),
        (dict(vocabulary=v, require=need, forbid=bad), ["mdt_smiles_check", "mdt_mol_graph", "mdt_sub_match", "mdt_screen_select_reject"]),
        (dict(vocabulary=v, kekulize=True), ["mdt_smiles_check", "mdt_mol_graph", "mdt_mol_hydrogens", "mdt_screen_select_reject"]),
        (dict(vocabulary=v, identity="graph", kekulize=True, require=need, forbid=bad, max_similarity=0.5),
         ["mdt_smiles_check", "mdt_mol_graph", "mdt_mol_hydrogens", "mdt_mol_key", "mdt_key_flags", "mdt_sub_match", "mdt_mol_fp",
          "mdt_screen_select_similar"]),
        (dict(vocabulary=v, known_tokens=known, identity="graph", forbid=bad, max_known_similarity=0.7, min_novelty=2),
         ["mdt_smiles_check", "mdt_mol_graph", "mdt_mol_key", "mdt_key_flags", "mdt_sub_match", "mdt_mol_fp", "mdt_fp_nearest",
          "mdt_edit_nearest", "mdt_screen_select_diverse_reject"])]
    known.mol_keys(v, "cpu"), known.fingerprints(v, "cpu")                   # (the known set's keys and fingerprints: once)
    for kw, want in today:
        logs = []
        for extra in (dict(), dict(limits=None)):
            assert run(**kw, **extra) == want, kw
            logs.append([(e[0], len(e), tuple(a for a in e[1:] if isinstance(a, int) and a < 4096)) for e in rec.log])
        assert logs[0] == logs[1]
        if "vocabulary" not in kw:
            continue
        # ... and limits= adds exactly one mdt_mol_rings, after the one mdt_mol_graph and the one mdt_mol_hydrogens
        got = run(**kw, limits=limits)
        assert got.count("mdt_mol_rings") == 1 and got.count("mdt_mol_hydrogens") == 1 and got.count("mdt_mol_graph") == 1, kw
        if "mdt_mol_hydrogens" in want:                                      # kekulize=True: its launch is the one that is used
            at = want.index("mdt_mol_hydrogens") + 1
            assert got == want[:at] + ["mdt_mol_rings"] + want[at:], kw
        elif "mdt_mol_graph" in want:
            at = want.index("mdt_mol_graph") + 1
            assert got == want[:at] + ["mdt_mol_hydrogens", "mdt_mol_rings"] + want[at:], kw
        else:
            assert got == [want[0], "mdt_mol_graph", "mdt_mol_hydrogens", "mdt_mol_rings"] + \
                [w if w.endswith("reject") else w + "_reject" for w in want[1:]], kw
        graph = rec.log[3 + got.index("mdt_mol_graph")]
        molh = rec.log[3 + got.index("mdt_mol_hydrogens")]
        ring = rec.log[3 + got.index("mdt_mol_rings")]
        assert len(ring) == 1 + 14 and ring[1:5] == graph[8:12] == molh[1:5] and ring[5] == molh[8]   # the one graph, its hydrogens
        assert ring[6:8] == (L_, N_ * G_) and 0 not in ring[8:14]            # lo, hi, three outputs and the flags: all given
        assert ring[8:10] == tuple(t.data_ptr() for t in limits.on("cpu"))
    # the public calls
    rec.log.clear()
    out = M.mol_rings(tok.to(torch.int16), v, "cpu")
    assert names(rec) == ["mdt_tokens_compact", "mdt_mol_graph", "mdt_mol_hydrogens", "mdt_mol_rings"]
    assert rec.log[3][6:10] == (L_, N_ * G_, 0, 0) and rec.log[3][5] == rec.log[2][8] and rec.log[2][7] == 4096
    assert [tuple(t.shape) for t in out] == [(N_ * G_, L_)] * 2 + [(N_ * G_, 16)] + [(N_ * G_,)] * 3 and all(t.dtype == torch.int64 for t in out)
    rec.log.clear()
    desc, verdict, status, position = M.mol_descriptors(tok, v, "cpu")
    assert names(rec) == ["mdt_tokens_compact", "mdt_mol_graph", "mdt_mol_hydrogens", "mdt_mol_rings"]
    assert desc.shape == (N_ * G_, 16) and all(t.dtype == torch.int64 and t.shape == (N_ * G_,) for t in (verdict, status, position))


def test_screen_candidates_forwards_limits_only_when_set(rec, monkeypatch):
    seen = {}

    class Inv:
        max_length = 32

        def sample_tokens(self, seq, device, **k):
            return torch.ones(seq.shape[0], 32, dtype=torch.long)
    monkeypatch.setattr(G, "screen_tokens", lambda *a, **k: seen.update(plain=k) or "plain")
    monkeypatch.setattr(G, "screen_tokens_diverse", lambda *a, **k: seen.update(diverse=k) or "diverse")
    cond, v, limits = torch.zeros(2, 12), vocabulary(), M.DescriptorLimits(max_rings=0)
    assert M.screen_candidates(Inv(), "fwd", cond, "dev", 3, 2, vocabulary=v, limits=limits) == "diverse"
    assert seen["diverse"] == dict(min_distance=1, min_novelty=1, vocabulary=v, limits=limits)
    assert M.screen_candidates(Inv(), "fwd", cond, "dev", 3, 2, vocabulary=v, limits=None) == "diverse"
    assert seen["diverse"] == dict(min_distance=1, min_novelty=1, vocabulary=v)
    assert M.screen_candidates(Inv(), "fwd", cond, "dev", 3, 2, limits=None) == "plain" and seen["plain"] == dict()
    assert rec.log == []


def test_refusals_come_before_anything_is_launched(rec):
    fwd, v = Fwd(rec), vocabulary()
    tok, cond = torch.ones(N_ * G_, L_, dtype=torch.long), torch.zeros(G_, n_)
    wide = torch.ones(N_ * G_, 65, dtype=torch.long)
    limits = M.DescriptorLimits(max_rings=0)
    div = lambda t=tok, **kw: M.screen_tokens_diverse(fwd, t, cond, "cpu", N_, K_, **kw)  # noqa: E731

    class Inv:
        max_length = 65

        def sample_tokens(self, *a, **k):
            raise AssertionError("sampled")
    for call, what in (
            (lambda: div(limits=limits), "give a vocabulary"),
            (lambda: div(wide, vocabulary=v, limits=limits), "at most 64"),
            (lambda: div(vocabulary=v, limits=dict(max_rings=0)), "DescriptorLimits"),
            (lambda: div(vocabulary=v, limits=True), "DescriptorLimits"),
            (lambda: M.screen_candidates(Inv(), fwd, cond, "cpu", N_, K_, vocabulary=v, limits=limits), "at most 64"),
            (lambda: M.screen_candidates(Inv(), fwd, cond, "cpu", N_, K_, limits=limits), "give a vocabulary"),
            (lambda: M.mol_rings(wide, v, "cpu"), "at most 64"),
            (lambda: M.mol_rings(tok.float(), v, "cpu"), "integer"),
            (lambda: M.mol_rings(tok, S.CHARS, "cpu"), "SmilesVocabulary"),
            (lambda: M.mol_descriptors(tok[:, :0], v, "cpu"), "at least one position"),
            (lambda: M.mol_descriptors(wide, v, "cpu"), "at most 64")):
        with pytest.raises(ValueError, match=what):
            call()
    assert rec.log == []
    with pytest.raises(TypeError):                                           # screen_tokens keeps its parameter list
        M.screen_tokens(fwd, tok, cond, "cpu", N_, K_, limits=limits)
    # the op refuses what the kernel does not take
    n, rows, h = torch.zeros(3, dtype=torch.int32), torch.zeros(3, 8, dtype=torch.int32), torch.zeros(3, 8, dtype=torch.uint8)
    b = torch.zeros(16, dtype=torch.int32)
    ring = torch.ops.mdt.mol_rings
    w65, h65 = torch.zeros(3, 65, dtype=torch.int32), torch.zeros(3, 65, dtype=torch.uint8)
    for call, what in ((lambda: ring(n, w65, n, w65, h65, None, None), "1 to 64"),
                       (lambda: ring(n, rows[:, :0], n, rows[:, :0], h[:, :0], None, None), "1 to 64"),
                       (lambda: ring(n, rows.long(), n, rows, h, None, None), "int32"), (lambda: ring(n[:2], rows, n, rows, h, None, None), "one value per row"),
                       (lambda: ring(n, rows, n, rows, h.int(), None, None), "uint8"), (lambda: ring(n, rows, n, rows, h[:, :4], None, None), "uint8"),
                       (lambda: ring(n, rows, n, rows, h, b, None), "together"), (lambda: ring(n, rows, n, rows, h, None, b), "together"),
                       (lambda: ring(n, rows, n, rows, h, b.long(), b), r"int32 \(16,\)"), (lambda: ring(n, rows, n, rows, h, b, b[:13]), r"int32 \(16,\)")):
        with pytest.raises(RuntimeError, match=what):
            call()
    assert rec.log == []


def test_public_surface_and_what_the_docstrings_promise():
    for name in ("mol_rings", "mol_descriptors", "DescriptorLimits", "DESCRIPTOR_NAMES"):
        assert getattr(M, name) is getattr(G, name)
    p = inspect.signature(M.screen_tokens_diverse).parameters
    assert p["limits"].default is None and list(p)[-1] == "screen_tokens_kwargs" and "limits" not in inspect.signature(M.screen_tokens).parameters
    assert list(inspect.signature(M.mol_rings).parameters) == list(inspect.signature(M.mol_descriptors).parameters) == ["tokens", "vocabulary", "device"]
    flat = " ".join(M.mol_rings.__doc__.split())
    for phrase in ("not RDKit's ring info and not an SSSR", "no envelope rings", "aromaticity is as written", "mdt::mol_hydrogens -> mdt::mol_rings"):
        assert phrase in flat, phrase
    flat = " ".join(M.mol_descriptors.__doc__.split())
    for phrase in ("No logP", "an aromatic-order bond is never rotatable", "milli-dalton"):
        assert phrase in flat, phrase
    flat = " ".join(M.screen_tokens_diverse.__doc__.split())
    for phrase in ("No status bit is free, so under ``limits=`` bit 128 also means", "that launch is made once when both are on",
                   "With None the call makes exactly the launches it makes without the keyword"):
        assert phrase in flat, phrase
