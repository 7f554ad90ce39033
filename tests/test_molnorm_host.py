"""No GPU: the definition of the normal form of a graph row (include/mdt_hip.h, mdt_mol_normalize) on its reference
(tests/molnorm_ref.py) -- the table written by hand, rows that pass through, pairs of spellings that get one key, respelling,
the Kekule view, idempotence, renumbering, an independent oracle (networkx: all shortest cycles through every ring bond) -- and the
plumbing: C export and argument checks, op schema and shape inference, the refusals, and the launch order of the public calls and
of the screening call with ``normalize`` on a recording library."""
import contextlib
import inspect
import os
import random
import re

import pytest
import torch

import molh_ref as H
import molkey_ref as K
import molnorm_ref as N
import molring_ref as R
import smiles_ref as S
from conftest import ROOT
import moleculediffusiontransformer_amd as M
from moleculediffusiontransformer_amd import generative as G, ops, runtime as rt


@pytest.fixture(scope="module")
def spelled():
    return K.random_spellings()


# ---------------------------------------------------------------------------------------------------------------------
# the definition on the reference
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", list(N.TABLE))
def test_the_hand_table(s):
    r = N.string_normal(s)
    want = set(range(r["n"])) if N.TABLE[s] == N.ALL else N.TABLE[s]
    assert r["molecule"] and r["verdict"] == 0 and len(s) <= 64
    assert r["aromatic"] == want
    assert r["flags"] & N.NORMALIZED and bool(r["flags"] & N.AROMATIC) == bool(want)
    atoms, bonds = N.unpacked(r)
    _, _, written, _ = K.graph(s)
    hydrogens = H.string_hydrogens(s)["hydrogens"]
    for x, (d, was) in enumerate(zip(atoms, written)):                       # bit 10 perceived, bracket bit set, H folded, the rest kept
        assert d >> 10 & 1 == int(x in want) and d >> 11 & 1 == 1 and d >> 17 & 15 == hydrogens[x]
        assert d & 0x3FF == was & 0x3FF and d >> 12 & 31 == was >> 12 & 31 and d >> 21 == was >> 21
    for (a, b, o), ring in zip(bonds, R.string_rings(s)["bond_ring"]):       # order 5 exactly inside one aromatic ring
        assert (o == 5) == any(a in ring_ and b in ring_ for ring_ in r["rings"]) and o in (1, 2, 3, 4, 5)
        assert o != 5 or ring


def test_what_the_table_must_hold():
    for s in ("c1ccccc1", "C1=CC=CC=C1", "c1ccncc1", "C1=CC=NC=C1", "c1cc[nH]c1", "C1=CNC=C1", "c1ccoc1", "C1=COC=C1", "c1c[nH]cn1",
              "C1=CNC=N1", "c1ccsc1", "C1=CC2=C(C=C1)C=CC=C2", "c1ccc2[nH]ccc2c1", "C1=CC=C2NC=CC2=C1", "[CH+]1C=CC=CC=C1",
              "c1ccc[cH+]cc1", "[CH-]1C=CC=C1", "C1=C[CH+]1", "c1ccccc1c1ccccc1", "C1=CC=CC=C1C1=CC=CC=C1", "O=c1cc[nH]cc1", "O=C1C=CNC=C1",
              "Cn1cnc2c1c(=O)n(C)c(=O)n2C", "CN1C=NC2=C1C(=O)N(C)C(=O)N2C", "[O-][n+]1ccccc1", "c1ccc2CCCCc2c1", "c1ccc2c(c1)Cc1ccccc12",
              "O=C1C=CC(=O)C=C1", "C1=CC=CC=CC=C1", "C1=CC=C1", "c1ccc1", "C1=CCC=C1", "c1ccc2cccc2cc1", "cc", "C1CCCCC1"):
        assert s in N.TABLE, s
    naphthalenes = [s for s in N.TABLE if sorted(H.string_hydrogens(s)["formula"][:3]) == [0, 8, 10] and N.TABLE[s] == N.ALL and "N" not in s.upper()]
    assert len(naphthalenes) >= 4                                            # aromatic and three Kekule structures
    assert N.TABLE["O=c1cc[nH]cc1"] == N.TABLE["O=C1C=CNC=C1"] == {1, 2, 3, 4, 5, 6}
    assert N.TABLE["Cn1cnc2c1c(=O)n(C)c(=O)n2C"] == {1, 2, 3, 4, 5, 6, 8, 10, 12} and N.TABLE["c1ccc2CCCCc2c1"] == {0, 1, 2, 3, 8, 9}
    assert N.TABLE["c1ccc2c(c1)Cc1ccccc12"] == set(range(13)) - {6} and N.TABLE["c1ccc2cccc2cc1"] == set()
    for s in ("c1ccccc1c1ccccc1", "C1=CC=CC=C1C1=CC=CC=C1"):                 # biphenyl: the axis stays order 1
        bonds = N.unpacked(N.string_normal(s))[1]
        assert bonds[6] == (5, 6, 1) and sorted(o for _, _, o in bonds) == [1] + [5] * 12
    cc = N.string_normal("cc")                                               # outside every ring: the Kekule structure that was found
    assert N.unpacked(cc)[1] == [(0, 1, 2)] and cc["flags"] == N.NORMALIZED | N.CHANGED and not any(d >> 10 & 1 for d in cc["atoms"])
    assert N.string_normal("C1CCCCC1")["flags"] == N.NORMALIZED and N.string_normal("c1ccccc1")["flags"] == N.NORMALIZED | N.AROMATIC
    assert N.string_normal("C1=CC=CC=C1")["flags"] == 7


def test_rows_that_are_not_normalised_pass_through():
    for s in ["", "C(", "C1CC", "c1ccccc", "Xx"] + [s for s, _ in S.MALFORMED_TABLE + S.OVERVALENT_TABLE]:
        r = N.string_normal(s[:64])
        assert not r["molecule"] and r["flags"] == 0 and not any(r["atoms"] + r["bonds"]), s
    for s in ("c1cccc1", "n1cccc1", "c1ccccc1c", "cF"):                      # verdict != 0: as written, flags 0
        r = N.string_normal(s)
        _, _, atoms, bonds = K.graph(s)
        assert r["molecule"] and r["verdict"] != 0 and r["flags"] == 0, s
        assert r["atoms"] == atoms + [0] * (64 - len(atoms)) and r["bonds"] == [N.pack(b) for b in bonds] + [0] * (64 - len(bonds))
    for row, named in N.special_rows():
        out = N.special_answer(row)
        width, n, nb, atoms, bonds = row[:5]
        assert out["flags"] == named["flags"] and out["aromatic"] == named.get("aromatic", out["aromatic"]), row[:3]
        assert len(out["atoms"]) == len(out["bonds"]) == width
        if not H.is_graph(n, nb, bonds, width):
            assert not any(out["atoms"] + out["bonds"])
    special = [N.special_answer(row) for row, _ in N.special_rows()]
    assert special[0]["atoms"][62] >> 10 & 1 == 0 and special[0]["bonds"][62] >> 16 == 1 and special[0]["bonds"][61] >> 16 == 5
    assert special[4]["bonds"][6] == N.pack((0, 0, 5))                       # an entry (x, x) at an atom of an aromatic ring
    assert special[6]["atoms"][0] >> 17 & 15 == 15 and [d >> 17 & 15 for d in special[7]["atoms"][:2]] == [15, 15]
    assert special[9]["bonds"][:2] == [N.pack((0, 1, 0)), N.pack((1, 2, 65535))]      # an order outside 1..5 stays


def test_pairs_that_differ_as_written_have_one_key_as_normal_forms():
    for a, b in N.PAIRS:
        assert K.string_key(a) != K.string_key(b) and K.string_key(a) and K.string_key(b), (a, b)
        assert N.normal_key(a) == N.normal_key(b) != 0, (a, b)
    for a, b in K.DIFFERENT_PAIRS:                                           # what differs as a molecule still differs
        if (a, b) != ("c1ccccc1", "C1=CC=CC=C1"):
            assert N.normal_key(a) != N.normal_key(b), (a, b)
    for a, b in K.EQUAL_PAIRS:
        assert N.normal_key(a) == N.normal_key(b) != 0, (a, b)
    assert N.normal_key("c1ccccc1") != N.normal_key("C1CCCCC1") != N.normal_key("C1=CCCCC1")
    assert N.normal_key("c1ccc2cccc2cc1") != 0 and N.normal_key("[CH3]") != N.normal_key("C")    # a radical is no methane


def test_the_four_spellings_of_every_random_graph_have_one_key(spelled):
    normalised = aromatic = 0
    for _, sp in spelled:
        keys = {N.normal_key(s) for s in sp}
        assert len(keys) == 1 and 0 not in keys, sp
        flags = {N.string_normal(s)["flags"] & 3 for s in sp}
        assert len(flags) == 1, sp
        normalised += 4 * (flags.pop() & 1)
        aromatic += sum(N.string_normal(s)["flags"] >> 1 & 1 for s in sp)
    print("strings normalised: %d, with an aromatic ring: %d" % (normalised, aromatic))
    assert len(spelled) == 500 and normalised > 1600 and aromatic > 400


def test_the_kekule_view_normalises_to_the_same_words_and_normalising_again_is_the_identity(spelled):
    views = again = 0
    for s in list(N.TABLE) + [s for _, sp in spelled for s in sp]:
        r = N.string_normal(s)
        if not r["flags"] & N.NORMALIZED:
            continue
        twice = N.again(r)
        assert (twice["atoms"], twice["bonds"]) == (r["atoms"], r["bonds"]) and twice["flags"] == r["flags"] & 3, s
        again += 1
        if r["flags"] & N.AROMATIC:
            atoms, bonds, _ = N.kekule_string_arrays(s)
            assert not any(d >> 10 & 1 for d in atoms) and all(o != 5 for _, _, o in bonds)
            view = N.special_answer(N.arrays_row(64, len(atoms), atoms, len(bonds), bonds))
            assert (view["atoms"], view["bonds"]) == (r["atoms"], r["bonds"]), s
            views += 1
    assert again > 1800 and views > 550


def test_a_renumbering_keeps_the_key_and_moves_the_aromatic_atoms(spelled):
    rng = random.Random(13)
    rows = [s for s in N.TABLE] + [sp[0] for _, sp in spelled[:240]]
    asked = 0
    for s in rows:
        r = N.string_normal(s)
        if not r["flags"] & N.NORMALIZED:
            continue
        _, _, atoms, bonds = K.graph(s)
        n, nb = len(atoms), len(bonds)
        to = list(range(n))
        rng.shuffle(to)                                                      # old atom a becomes to[a]
        order = list(range(nb))
        rng.shuffle(order)
        new_atoms = [0] * n
        for a in range(n):
            new_atoms[to[a]] = atoms[a]
        new_bonds = []
        for e in order:
            a, b, o = bonds[e]
            new_bonds.append((to[b], to[a], o) if rng.random() < 0.5 else (to[a], to[b], o))
        out = N.special_answer(N.arrays_row(64, n, new_atoms, nb, new_bonds))
        out.update(n=n, nb=nb)
        assert out["flags"] & 3 == r["flags"] & 3, s
        assert K.key(*N.unpacked(out)) == K.key(*N.unpacked(r)), s
        assert out["aromatic"] == {to[a] for a in r["aromatic"]}, s
        asked += 1
    assert asked >= 240


def test_an_independent_oracle_on_every_molecule_row(spelled):
    """networkx: for every ring bond ALL shortest cycles through it.  Every ring the reference tried is one of them; where no bond
    has more than two, the aromatic atoms are those of judging all of them.  Rows with a bond in three or more are counted."""
    import networkx as nx
    rows = list(N.TABLE) + [s for _, sp in spelled for s in sp] + [s[:64] for s in S.mutated_rows(512)]
    asked = left_out = aromatic_rows = 0
    for s in rows:
        r = N.string_normal(s)
        if not r["flags"] & N.NORMALIZED:
            continue
        _, _, atoms, bonds = K.graph(s)
        h = H.string_hydrogens(s)
        p = N.pi_electrons(len(atoms), atoms, bonds, N.kekule_orders(bonds, h["partner"]), h["hydrogens"], R.string_rings(s)["bond_ring"])
        g = nx.Graph()
        g.add_nodes_from(range(len(atoms)))
        g.add_edges_from((a, b) for a, b, _ in bonds if a != b)
        bridges = {frozenset(e) for e in nx.bridges(g)}
        cycles, most = set(), 0
        for a, b in g.edges:
            if frozenset((a, b)) in bridges:
                continue
            cut = g.copy()
            cut.remove_edge(a, b)
            through = {frozenset(path) for path in nx.all_shortest_paths(cut, a, b)}
            most = max(most, len(through))
            cycles |= through
        asked += 1
        assert set(r["tried"]) <= cycles, s
        if most > 2:
            left_out += 1
            continue
        want = set()
        for ring in cycles:
            if all(p[x] is not None for x in ring) and sum(p[x] for x in ring) % 4 == 2:
                want |= ring
        assert r["aromatic"] == want, s
        aromatic_rows += bool(want)
    print("molecule rows asked: %d, left out (a bond in three or more smallest cycles): %d, aromatic: %d" % (asked, left_out, aromatic_rows))
    assert asked >= 2000 and left_out <= 0.02 * asked and aromatic_rows > 500


# ---------------------------------------------------------------------------------------------------------------------
# header, library, binding
# ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_the_library_exports_the_new_symbol():
    hdr = open(os.path.join(ROOT, "include", "mdt_hip.h")).read()
    lib = rt.load_library()
    assert re.search(r"\bint mdt_mol_normalize\s*\(", hdr) and "mdt_mol_normalize" in rt.SYMBOLS and hasattr(lib, "mdt_mol_normalize")
    assert len(rt.SYMBOLS["mdt_mol_normalize"][1]) == 14
    assert int(re.search(r"#define MDT_ABI_VERSION (\d+)", hdr).group(1)) == rt.ABI_VERSION == 5 == lib.mdt_abi_version()
    for name, value in (("NORMALIZED", N.NORMALIZED), ("AROMATIC", N.AROMATIC), ("CHANGED", N.CHANGED)):
        assert int(re.search(r"\bMDT_MOLN_%s = (\d+)" % name, hdr).group(1)) == value == getattr(rt, "MOLN_" + name)
    flat = " ".join(hdr.replace(" * ", " ").split())
    for phrase in ("Not RDKit's aromaticity model", "no envelope rings", "is NOT aromatic here, and RDKit says it is",
                   "A bond in three or more equally small cycles (cubane-like) may try numbering-dependent rings",
                   "A lower-case atom outside every perceived ring keeps the Kekule structure that mdt_mol_hydrogens found",
                   "No tautomers, no charge normalisation", "no stereo", "B 13, C 14, N and P 15, O and S 16", "there is no step cap",
                   "no aromaticity perception (C1=CC=CC=C1 and c1ccccc1 differ)", "Aromaticity is as written"):
        assert phrase in flat, phrase
    assert "k_molnorm.hip" in [s for s, _ in __import__("moleculediffusiontransformer_amd.build", fromlist=["SOURCES"]).SOURCES]
    src = open(os.path.join(ROOT, "moleculediffusiontransformer_amd", "csrc", "k_molnorm.hip")).read()
    for used in ("moln_pi(", "moln_hueckel(", "moln_atom_word(", "moln_bond_word(", "mol_graph_ok_wave(", "mdt_molnorm.h", "mdt_finish("):
        assert used in src, used
    assert "__shared__" not in src and "__syncthreads" not in src            # no LDS, no barrier
    shared = open(os.path.join(ROOT, "moleculediffusiontransformer_amd", "csrc", "mdt_molnorm.h")).read()
    assert "mdt_molh.h" in shared and "molh_charge(" in shared and "molh_charge(uint32_t" not in shared   # reused, not copied
    assert "mdt_molrow.h" in shared and "int mol_search(" not in shared and "int mol_highest(" not in shared
    for used in ("mol_search(", "mol_ring_adj(", "mol_highest(", "mol_lowest(", "mol_popc("):
        assert used in shared, used


def test_entry_point_refuses_bad_arguments_before_any_launch():
    lib = rt.load_library()

    def call(L=32, R_=5, p=8, out=8, **one):
        a = dict(natoms=p, atoms=p, nbonds=p, bonds=p, hydrogens=p, partner=p, verdict=p, bond_ring=p, out_atoms=out, out_bonds=out, flags=out)
        a.update(one)
        return lib.mdt_mol_normalize(a["natoms"], a["atoms"], a["nbonds"], a["bonds"], a["hydrogens"], a["partner"], a["verdict"],
                                     a["bond_ring"], L, R_, a["out_atoms"], a["out_bonds"], a["flags"], 0)
    cases = [(dict(L=0), b"L <= 64"), (dict(L=65), b"L <= 64"), (dict(R_=-1), b"R >= 0"), (dict(p=0), b"null"), (dict(out=0), b"null")]
    cases += [({name: 0}, b"null") for name in ("natoms", "atoms", "nbonds", "bonds", "hydrogens", "partner", "verdict", "bond_ring",
                                                "out_atoms", "out_bonds", "flags")]
    for kw, what in cases:
        assert call(**kw) == 2, kw
        assert what in lib.mdt_last_error(), (kw, lib.mdt_last_error())
    assert call(R_=0) == 0 and call(R_=0, p=0, out=0) == 0                   # nothing to do: nothing is launched or read
    assert call(R_=0, L=65) != 0 and call(R_=0, L=0) != 0


def vocabulary():
    return M.SmilesVocabulary([None] + S.CHARS)


def test_op_schema_and_shape_inference():
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert str(torch.ops.mdt.mol_normalize.default._schema) == \
        ("mdt::mol_normalize(Tensor natoms, Tensor atoms, Tensor nbonds, Tensor bonds, Tensor hydrogens, Tensor partner, Tensor verdict, "
         "Tensor bond_ring) -> (Tensor, Tensor, Tensor)")
    with FakeTensorMode():
        n, rows, h, v = (torch.empty(15, dtype=torch.int32), torch.empty(15, 40, dtype=torch.int32), torch.empty(15, 40, dtype=torch.uint8),
                         torch.empty(15, dtype=torch.uint8))
        out = torch.ops.mdt.mol_normalize(n, rows, n, rows, h, h, v, h)
        assert [(tuple(t.shape), t.dtype) for t in out] == [((15, 40), torch.int32), ((15, 40), torch.int32), ((15,), torch.uint8)]
    n, rows, h, v = (torch.zeros(3, dtype=torch.int32), torch.zeros(3, 4, dtype=torch.int32), torch.zeros(3, 4, dtype=torch.uint8),
                     torch.zeros(3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU implementation"):          # no CPU implementation behind the op
        torch.ops.mdt.mol_normalize(n, rows, n, rows, h, h, v, h)


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


def test_launch_order_of_the_public_calls_with_and_without_normalize(rec):
    tok, v = torch.ones(N_ * G_, L_, dtype=torch.long), vocabulary()
    known = M.KnownSet(torch.ones(4, L_, dtype=torch.long), L_)
    frag = M.SubstructureSet(["c1ccccc1", "[CH4]"], v)
    frag.on("cpu")
    head = ["mdt_tokens_compact", "mdt_mol_graph"]
    for call, tail in ((lambda **kw: M.mol_key(tok, v, "cpu", **kw), ["mdt_mol_key"]),
                       (lambda **kw: M.mol_fingerprint(tok, v, "cpu", 1, **kw), ["mdt_mol_fp"])):
        logs = []
        for kw in (dict(), dict(normalize=False)):                           # False: the launches made today
            rec.log.clear()
            call(**kw)
            assert names(rec) == head + tail
            logs.append(shape_of(rec))
        assert logs[0] == logs[1]
        rec.log.clear()
        call(normalize=True)
        assert names(rec) == head + FORM + tail
        graph, molh, ring, norm, last = rec.log[1:6]
        assert norm[1:5] == graph[8:12] == molh[1:5] == ring[1:5] and norm[5:8] == molh[8:11] and norm[8] == ring[10]
        assert norm[9:11] == (L_, N_ * G_) and ring[8:10] == (0, 0) and 0 not in norm[11:14]
        assert (last[1], last[3]) == (graph[8], graph[10]) and (last[2], last[4]) == (norm[11], norm[12])   # natoms, nbonds reused
    rec.log.clear()
    M.tanimoto(tok, tok, v, "cpu")
    assert names(rec) == (head + ["mdt_mol_fp"]) * 2 + ["mdt_fp_tanimoto_rows"]
    rec.log.clear()
    M.tanimoto(tok, tok, v, "cpu", normalize=True)
    assert names(rec) == (head + FORM + ["mdt_mol_fp"]) * 2 + ["mdt_fp_tanimoto_rows"]
    # the known set: keys and fingerprints of normal forms are cached apart from those as written
    for get, last in ((lambda **kw: known.mol_keys(v, "cpu", **kw), "mdt_mol_key"), (lambda **kw: known.fingerprints(v, "cpu", 2, **kw), "mdt_mol_fp")):
        rec.log.clear()
        plain = get()
        assert names(rec) == ["mdt_mol_graph", last]
        rec.log.clear()
        normal = get(normalize=True)
        assert names(rec) == ["mdt_mol_graph"] + FORM + [last]
        rec.log.clear()
        assert get() is plain and get(normalize=False) is plain and get(normalize=True) is normal and rec.log == []
    rec.log.clear()
    M.nearest_known_tanimoto(tok, known, v, "cpu")
    assert names(rec) == head + ["mdt_mol_fp", "mdt_fp_nearest"]
    rec.log.clear()
    M.nearest_known_tanimoto(tok, known, v, "cpu", normalize=True)
    assert names(rec) == head + FORM + ["mdt_mol_fp", "mdt_fp_nearest"]
    assert rec.log[-1][3] == known.fingerprints(v, "cpu", 2, normalize=True)[0].data_ptr() != known.fingerprints(v, "cpu", 2)[0].data_ptr()
    rec.log.clear()
    M.has_substructure(tok, frag, v, "cpu")
    assert names(rec) == head + ["mdt_sub_match"]
    rec.log.clear()
    out = M.has_substructure_normalized(tok, frag, v, "cpu")
    assert names(rec) == head + FORM + ["mdt_sub_match"]
    assert rec.log[-1][2] == rec.log[4][11] and rec.log[-1][4] == rec.log[4][12] and rec.log[-1][8] == frag.on("cpu")[1].data_ptr()
    assert [tuple(t.shape) for t in out] == [(N_ * G_, 2)] * 2 + [(N_ * G_,)] * 2
    rec.log.clear()
    out = M.mol_normalize(tok.to(torch.int16), v, "cpu")
    assert names(rec) == head + FORM and rec.log[2][7] == 4096
    assert [tuple(t.shape) for t in out] == [(N_ * G_,), (N_ * G_, L_), (N_ * G_,), (N_ * G_, L_)] + [(N_ * G_,)] * 4
    assert all(t.dtype == torch.int64 for t in out)


def test_launch_order_of_the_screening_call_with_and_without_normalize(rec):
    tok, cond, v = torch.ones(N_ * G_, L_, dtype=torch.long), torch.zeros(G_, n_), vocabulary()
    known = M.KnownSet(torch.ones(4, L_, dtype=torch.long), L_)
    need, bad = M.SubstructureSet(["C=O", "N"], v), M.SubstructureSet(["C#N", "OO", "c1ccccc1"], v)
    need.on("cpu"), bad.on("cpu")
    limits = M.DescriptorLimits.lipinski()
    run = lambda **kw: (rec.log.clear(), M.screen_tokens_diverse(Fwd(rec), tok, cond, "cpu", N_, K_, **kw), names(rec)[3:])[2]  # noqa: E731
    today = [
        (dict(), ["mdt_screen_select"]),
        (dict(vocabulary=v), ["mdt_smiles_check", "mdt_screen_select_reject"]),
        (dict(known_tokens=known, min_novelty=2), ["mdt_edit_nearest", "mdt_screen_select_diverse"]),
        (dict(vocabulary=v, identity="graph"), ["mdt_smiles_check", "mdt_mol_graph", "mdt_mol_key", "mdt_key_flags", "mdt_screen_select_reject"]),
        (dict(vocabulary=v, max_similarity=0.5), ["mdt_smiles_check", "mdt_mol_graph", "mdt_mol_fp", "mdt_screen_select_similar"]),
        (dict(vocabulary=v, require=need, forbid=bad), ["mdt_smiles_check", "mdt_mol_graph", "mdt_sub_match", "mdt_screen_select_reject"]),
        (dict(vocabulary=v, kekulize=True), ["mdt_smiles_check", "mdt_mol_graph", "mdt_mol_hydrogens", "mdt_screen_select_reject"]),
        (dict(vocabulary=v, limits=limits), ["mdt_smiles_check", "mdt_mol_graph", "mdt_mol_hydrogens", "mdt_mol_rings", "mdt_screen_select_reject"]),
        (dict(vocabulary=v, identity="graph", kekulize=True, require=need, forbid=bad, max_similarity=0.5),
         ["mdt_smiles_check", "mdt_mol_graph", "mdt_mol_hydrogens", "mdt_mol_key", "mdt_key_flags", "mdt_sub_match", "mdt_mol_fp",
          "mdt_screen_select_similar"]),
        (dict(vocabulary=v, identity="graph", limits=limits, forbid=bad),
         ["mdt_smiles_check", "mdt_mol_graph", "mdt_mol_hydrogens", "mdt_mol_rings", "mdt_mol_key", "mdt_key_flags", "mdt_sub_match",
          "mdt_screen_select_reject"]),
        (dict(vocabulary=v, known_tokens=known, identity="graph", forbid=bad, max_known_similarity=0.7, min_novelty=2, kekulize=True, limits=limits),
         ["mdt_smiles_check", "mdt_mol_graph", "mdt_mol_hydrogens", "mdt_mol_rings", "mdt_mol_key", "mdt_key_flags", "mdt_sub_match",
          "mdt_mol_fp", "mdt_fp_nearest", "mdt_edit_nearest", "mdt_screen_select_diverse_reject"])]
    for normal in (False, True):                                             # (the known set's keys and fingerprints: once)
        known.mol_keys(v, "cpu", normalize=normal), known.fingerprints(v, "cpu", normalize=normal)
    asked, keys_of = [], known.mol_keys
    known.mol_keys = lambda *a, **k: asked.append(k) or keys_of(*a, **k)
    for kw, want in today:
        logs = []
        del asked[:]
        for extra in (dict(), dict(normalize=False)):                        # False: the launches made today, argument for argument
            assert run(**kw, **extra) == want, kw
            logs.append(shape_of(rec))
        assert logs[0] == logs[1]
        consumers = [w for w in want if w in ("mdt_mol_key", "mdt_sub_match", "mdt_mol_fp")]
        if not consumers:
            continue
        # normalize=True: one mol_graph, one mol_hydrogens, one mol_rings -- those kekulize / limits make -- then one mol_normalize
        got = run(**kw, normalize=True)
        for one in ("mdt_mol_graph", "mdt_mol_hydrogens", "mdt_mol_rings", "mdt_mol_normalize"):
            assert got.count(one) == 1, (kw, one)
        at = want.index("mdt_mol_graph") + 1
        rest = [w for w in want[at:] if w not in ("mdt_mol_hydrogens", "mdt_mol_rings")]
        assert got == want[:at] + FORM + rest, kw
        at = {name: rec.log[3 + got.index(name)] for name in got}
        graph, molh, ring, norm = at["mdt_mol_graph"], at["mdt_mol_hydrogens"], at["mdt_mol_rings"], at["mdt_mol_normalize"]
        assert norm[1:5] == graph[8:12] == molh[1:5] == ring[1:5] and norm[5:8] == molh[8:11] and norm[8] == ring[10]
        assert norm[9:11] == (L_, N_ * G_) and 0 not in norm[11:14]
        given = tuple(t.data_ptr() for t in limits.on("cpu")) if "limits" in kw else (0, 0)
        assert ring[8:10] == given                                           # limits still reads the graph as written, in that launch
        for name in consumers:                                               # the consumers read the normal form, counts reused
            assert (at[name][1], at[name][3]) == (graph[8], graph[10]) and (at[name][2], at[name][4]) == (norm[11], norm[12]), (kw, name)
        if "mdt_key_flags" in got and "known_tokens" in kw:                  # (no key is non-zero here: ask which keys were taken)
            assert asked[-1] == dict(normalize=True) and dict(normalize=True) not in asked[:-1]
        if "mdt_fp_nearest" in got:
            assert at["mdt_fp_nearest"][3] == known.fingerprints(v, "cpu", normalize=True)[0].data_ptr()


def test_screen_candidates_forwards_normalize_only_when_set(rec, monkeypatch):
    seen = {}

    class Inv:
        max_length = 32

        def sample_tokens(self, seq, device, **k):
            return torch.ones(seq.shape[0], 32, dtype=torch.long)
    monkeypatch.setattr(G, "screen_tokens", lambda *a, **k: seen.update(plain=k) or "plain")
    monkeypatch.setattr(G, "screen_tokens_diverse", lambda *a, **k: seen.update(diverse=k) or "diverse")
    cond, v = torch.zeros(2, 12), vocabulary()
    assert M.screen_candidates(Inv(), "fwd", cond, "dev", 3, 2, vocabulary=v, identity="graph", normalize=True) == "diverse"
    assert seen["diverse"] == dict(min_distance=1, min_novelty=1, vocabulary=v, identity="graph", normalize=True)
    assert M.screen_candidates(Inv(), "fwd", cond, "dev", 3, 2, vocabulary=v, identity="graph", normalize=False) == "diverse"
    assert seen["diverse"] == dict(min_distance=1, min_novelty=1, vocabulary=v, identity="graph")
    assert M.screen_candidates(Inv(), "fwd", cond, "dev", 3, 2, normalize=False) == "plain" and seen["plain"] == dict()
    assert rec.log == []


def test_refusals_come_before_anything_is_launched(rec):
    fwd, v = Fwd(rec), vocabulary()
    tok, cond = torch.ones(N_ * G_, L_, dtype=torch.long), torch.zeros(G_, n_)
    wide = torch.ones(N_ * G_, 65, dtype=torch.long)
    known = M.KnownSet(torch.ones(4, L_, dtype=torch.long), L_)
    div = lambda t=tok, **kw: M.screen_tokens_diverse(fwd, t, cond, "cpu", N_, K_, **kw)  # noqa: E731

    class Inv:
        max_length = 65

        def sample_tokens(self, *a, **k):
            raise AssertionError("sampled")

    class Inv32(Inv):
        max_length = 32
    for call, what in (
            (lambda: div(normalize=True), "give a vocabulary"),
            (lambda: div(wide, vocabulary=v, identity="string", normalize=True), "at most 64"),
            (lambda: div(vocabulary=v, normalize=True), "ask for one of them"),
            (lambda: div(vocabulary=v, normalize=True, kekulize=True, limits=M.DescriptorLimits(max_rings=0)), "ask for one of them"),
            (lambda: div(vocabulary=v, identity="graph", normalize=1), "True or False"),
            (lambda: div(vocabulary=v, identity="graph", normalize=None), "True or False"),
            (lambda: M.screen_candidates(Inv(), fwd, cond, "cpu", N_, K_, vocabulary=v, normalize=True), "at most 64"),
            (lambda: M.screen_candidates(Inv32(), fwd, cond, "cpu", N_, K_, vocabulary=v, normalize=True), "ask for one of them"),
            (lambda: M.screen_candidates(Inv32(), fwd, cond, "cpu", N_, K_, normalize=True), "give a vocabulary"),
            (lambda: M.mol_normalize(wide, v, "cpu"), "at most 64"),
            (lambda: M.mol_normalize(tok.float(), v, "cpu"), "integer"),
            (lambda: M.mol_normalize(tok, S.CHARS, "cpu"), "SmilesVocabulary"),
            (lambda: M.mol_normalize(tok[:, :0], v, "cpu"), "at least one position"),
            (lambda: M.mol_key(tok, v, "cpu", normalize="yes"), "True or False"),
            (lambda: M.mol_fingerprint(tok, v, "cpu", normalize=0), "True or False"),
            (lambda: M.tanimoto(tok, tok, v, "cpu", normalize=1), "True or False"),
            (lambda: M.nearest_known_tanimoto(tok, known, v, "cpu", normalize=1), "True or False"),
            (lambda: known.mol_keys(v, "cpu", normalize=1), "True or False"),
            (lambda: known.fingerprints(v, "cpu", normalize=1), "True or False"),
            (lambda: M.has_substructure_normalized(wide, ["C"], v, "cpu"), "at most 64"),
            (lambda: M.has_substructure_normalized(tok, [], v, "cpu"), "patterns")):
        with pytest.raises(ValueError, match=what):
            call()
    assert rec.log == []
    with pytest.raises(TypeError):                                           # screen_tokens keeps its parameter list
        M.screen_tokens(fwd, tok, cond, "cpu", N_, K_, normalize=True)
    with pytest.raises(TypeError):                                           # keyword-only
        M.mol_key(tok, v, "cpu", True)
    # the op refuses what the kernel does not take
    n, rows, h, d = (torch.zeros(3, dtype=torch.int32), torch.zeros(3, 8, dtype=torch.int32), torch.zeros(3, 8, dtype=torch.uint8),
                     torch.zeros(3, dtype=torch.uint8))
    form = torch.ops.mdt.mol_normalize
    w65, h65 = torch.zeros(3, 65, dtype=torch.int32), torch.zeros(3, 65, dtype=torch.uint8)
    for call, what in ((lambda: form(n, w65, n, w65, h65, h65, d, h65), "1 to 64"),
                       (lambda: form(n, rows[:, :0], n, rows[:, :0], h[:, :0], h[:, :0], d, h[:, :0]), "1 to 64"),
                       (lambda: form(n, rows.long(), n, rows, h, h, d, h), "int32"), (lambda: form(n[:2], rows, n, rows, h, h, d, h), "one value per row"),
                       (lambda: form(n, rows, n, rows, h.int(), h, d, h), "hydrogens must be uint8"),
                       (lambda: form(n, rows, n, rows, h, h[:, :4], d, h), "partner must be uint8"),
                       (lambda: form(n, rows, n, rows, h, h, d.int(), h), "verdict must be uint8"),
                       (lambda: form(n, rows, n, rows, h, h, d[:2], h), "verdict must be uint8"),
                       (lambda: form(n, rows, n, rows, h, h, d, h.int()), "bond_ring must be uint8"),
                       (lambda: form(n, rows, n, rows, h, h, d, h[:2]), "bond_ring must be uint8")):
        with pytest.raises(RuntimeError, match=what):
            call()
    assert rec.log == []


def test_public_surface_and_what_the_docstrings_promise():
    for name in ("mol_normalize", "has_substructure_normalized"):
        assert getattr(M, name) is getattr(G, name)
    for f in (M.mol_key, M.mol_fingerprint, M.tanimoto, M.nearest_known_tanimoto, M.KnownSet.mol_keys, M.KnownSet.fingerprints):
        p = inspect.signature(f).parameters["normalize"]
        assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY, f
    p = inspect.signature(M.screen_tokens_diverse).parameters
    assert p["normalize"].default is False and list(p)[-2:] == ["normalize", "screen_tokens_kwargs"]
    assert "normalize" not in inspect.signature(M.screen_tokens).parameters
    assert list(inspect.signature(M.has_substructure).parameters) == list(inspect.signature(M.has_substructure_normalized).parameters) == \
        ["tokens", "patterns", "vocabulary", "device"]
    assert list(inspect.signature(M.mol_normalize).parameters) == ["tokens", "vocabulary", "device"]
    flat = " ".join(M.mol_normalize.__doc__.split())
    for phrase in ("not RDKit's aromaticity model", "no envelope rings", "azulene is NOT aromatic here, and RDKit says it is",
                   "A bond in three or more equally small cycles (cubane-like) may try numbering-dependent rings",
                   "A lower-case atom outside every perceived ring keeps the Kekule structure", "No tautomers, no charge normalisation, no stereo",
                   "mdt::mol_hydrogens -> mdt::mol_rings -> mdt::mol_normalize"):
        assert phrase in flat, phrase
    flat = " ".join(M.has_substructure_normalized.__doc__.split())
    for phrase in ("AROMATIC FRAGMENTS MUST BE WRITTEN IN LOWER CASE", "[CH4] now accepts C", "[nH] accepts the N of C1=CNC=C1", "matched as written"):
        assert phrase in flat, phrase
    for f, old in ((M.mol_key, "no aromaticity perception"), (M.mol_fingerprint, "no aromaticity perception"),
                   (M.has_substructure, "[CH4] does not accept C"), (M.tanimoto, "no aromaticity perception")):
        flat = " ".join(f.__doc__.split())
        assert old in flat and "ormali" in flat, f                            # the old limit stays, and points to the way round it
    flat = " ".join(M.screen_tokens_diverse.__doc__.split())
    for phrase in ("never a second one", "``limits`` still reads the graph as written", "at least one consumer",
                   "With False (the default) the call makes exactly the launches it makes without the keyword"):
        assert phrase in flat, phrase
