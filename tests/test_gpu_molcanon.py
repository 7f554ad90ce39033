"""-m gpu: mdt_mol_canon (csrc/k_molcanon.hip), mol_canon(), mol_same() and the canonical=True spellings on the device.  Every
comparison is exact: the priority, the relabelled arrays, the flags and the node counts against the plain-int reference
tests/molcanon_ref.py, the written rows against tests/molwrite_ref.py walked in that priority.  The longest row here is
hexaphenylethane, which stops at the node cap."""
import random

import pytest
import torch

import molcanon_ref as Q
import molkey_ref as K
import molnorm_ref as N
import molscaf_ref as C
import molwrite_ref as W
import smiles_ref as S
from gpu_util import DEV
from moleculediffusiontransformer_amd import (SmilesVocabulary, mol_canon, mol_respell, mol_same, mol_write, runtime as rt, scaffold_keep)
from moleculediffusiontransformer_amd import ops  # noqa: F401  (registers torch.ops.mdt.*)

pytestmark = pytest.mark.gpu

SYMMETRIC = ["C12C3C4C1C5C2C3C45", "C12C3C1C1C4C2C3C41", "C12C3C1C1C2C31", "C1C2CC3CC1CC(C2)C3", "c1ccc(cc1)-c1ccccc1", "c1ccc2ccccc2c1",
             "c1ccc2cc3ccccc3cc2c1", "c1cc2ccc3cccc4ccc(c1)c2c34", "C1CCC2(CC1)CCCCC2", "C1CC2CCC1C2", "C1CC2CCC1CC2",
             "OC(=O)CC(O)(CC(O)=O)C(O)=O", "C1CC1.C1CC1", "C12C3C4C1C5C2C3C45.C12C3C4C1C5C2C3C45",
             "c1ccccc1", "C1CCCCC1", "CC(C)(C)C", "C1CC1", "C12C3C1C23", "Cc1cc(C)cc(C)c1", "Cc1ccc(C)cc1", "ClC(Cl)(Cl)Cl",
             "FC(F)(F)C(F)(F)F", "O=C=O", "C1COCCO1", "C1CCC2CCCCC2C1", "C1CCCCC1C1CCCCC1", "CC.CC.CC", "c1ccc2c(c1)c1ccccc1c1ccccc21",
             "[NH4+].[Cl-].[NH4+].[Cl-]"]
CORONENE = "c1cc2ccc3ccc4ccc5ccc6ccc1c1c2c3c4c5c61"
HEXAPHENYLBENZENE = "c1ccccc1c1c(c2ccccc2)c(c2ccccc2)c(c2ccccc2)c(c2ccccc2)c1c1ccccc1"
DODECAHEDRANE = "C12C3C4C5C1C1C6C2C2C3C3C4C4C5C1C1C6C2C3C41"
HEXAPHENYLETHANE = "c1ccccc1C(c1ccccc1)(c1ccccc1)C(c1ccccc1)(c1ccccc1)c1ccccc1"
LARGE = SYMMETRIC + [CORONENE, HEXAPHENYLBENZENE, DODECAHEDRANE, HEXAPHENYLETHANE, ".".join(["[Cl-]"] * 8), "", "C(", "CCO"]
MASK32 = 0xFFFFFFFF


@pytest.fixture(scope="module")
def spelled():
    return K.random_spellings()


@pytest.fixture(scope="module")
def vocab(spelled):
    used = "".join(LARGE) + "".join(C.TABLE) + "".join(s for _, sp in spelled for s in sp)
    return SmilesVocabulary([None] + sorted(set(S.CHARS) | set(used) | set("$:*%\\/csnopbBPSI")))


def graph_of(strings, vocabulary, width):
    packed, n, _, _ = torch.ops.mdt.tokens_compact(vocabulary.encode(strings, width).to(DEV), 0, 1.0)
    return torch.ops.mdt.mol_graph(packed, n, *vocabulary.on(DEV))[:4]


def device_arrays(rows, width):
    """rows: [(n, atoms, nb, bonds as (a, b, order))] -> the four graph arrays on the device, garbage beyond the lists"""
    natoms = torch.tensor([r[0] for r in rows], dtype=torch.int32, device=DEV)
    nbonds = torch.tensor([r[2] for r in rows], dtype=torch.int32, device=DEV)
    atoms = torch.full((len(rows), width), 0x7FFFFFFF, dtype=torch.int32)   # (beyond the counts: never read)
    bonds = torch.full((len(rows), width), 0x7FFFFFFF, dtype=torch.int32)
    signed = lambda w: w - (1 << 32 if w >> 31 else 0)  # noqa: E731
    for r, (_, la, _, lb) in enumerate(rows):
        la, lb = list(la)[:width], list(lb)[:width]
        if la:
            atoms[r, :len(la)] = torch.tensor([signed(w) for w in la], dtype=torch.int32)
        if lb:
            bonds[r, :len(lb)] = torch.tensor([signed(N.pack(e)) for e in lb], dtype=torch.int32)
    return natoms, atoms.to(DEV), nbonds, bonds.to(DEV)


def words(t):
    return [[int(x) & MASK32 for x in row] for row in t.tolist()]


def compare(got, want, what):
    """got: the op's five outputs; want: the reference's answers.  Word for word; nodes where the row is decided."""
    priority, canon_atoms, canon_bonds, nodes, flags = got
    torch.cuda.synchronize()
    assert [t.dtype for t in got] == [torch.int64, torch.int32, torch.int32, torch.int32, torch.uint8]
    assert flags.tolist() == [r["flags"] for r in want], what
    assert priority.tolist() == [r["priority"] for r in want], what
    assert words(canon_atoms) == [r["canon_atoms"] for r in want] and words(canon_bonds) == [r["canon_bonds"] for r in want], what
    for got_nodes, r in zip(nodes.tolist(), want):
        assert (got_nodes > Q.MAX_NODES) if r["flags"] == Q.UNDECIDED else (got_nodes == r["nodes"]), (what, got_nodes, r["nodes"])


def renumbered(atoms, bonds, rng):
    to = list(range(len(atoms)))
    rng.shuffle(to)
    new_atoms = [0] * len(atoms)
    for a, d in enumerate(atoms):
        new_atoms[to[a]] = d
    new_bonds = [(to[a], to[b], o) if rng.random() < 0.5 else (to[b], to[a], o) for a, b, o in bonds]
    rng.shuffle(new_bonds)
    return new_atoms, new_bonds


def test_the_symmetric_table_and_the_large_rows(vocab):
    want = [Q.string_canon(s) for s in LARGE]
    compare(torch.ops.mdt.mol_canon(*graph_of(LARGE, vocab, 64)), want, "large")
    by = dict(zip(LARGE, want))
    assert (by[HEXAPHENYLBENZENE]["leaves"], by[DODECAHEDRANE]["leaves"], by[CORONENE]["leaves"]) == (768, 120, 12)
    assert by[HEXAPHENYLETHANE]["flags"] == Q.UNDECIDED and by["C12C3C4C1C5C2C3C45.C12C3C4C1C5C2C3C45"]["nodes"] == 2 * by["C12C3C4C1C5C2C3C45"]["nodes"]
    assert [r["flags"] for r in want].count(Q.CANONICAL) == len(LARGE) - 3 and by[""]["flags"] == by["C("]["flags"] == 0


def test_the_random_spellings_at_width_32(spelled):
    rows = []
    for _, sp in spelled:
        for s in sp:
            _, _, atoms, bonds = K.graph(s)
            rows.append((len(atoms), atoms, len(bonds), bonds))
    want = [Q.canon(*r, 32) for r in rows]
    compare(torch.ops.mdt.mol_canon(*device_arrays(rows, 32)), want, "spellings")
    assert len(rows) == 2000 and all(r["flags"] == Q.CANONICAL for r in want)
    for g in range(500):
        assert len({Q.form(r) for r in want[4 * g:4 * g + 4]}) == 1, g
    print("nodes: 1 in %d rows, at most %d" % (sum(r["nodes"] == 1 for r in want), max(r["nodes"] for r in want)))


@pytest.mark.parametrize("width", [8, 28, 64])
def test_the_edge_rows_over_a_prefilled_output(width):
    """Through the C ABI on outputs pre-filled with a pattern and followed by a guard: every word defined, the guard untouched."""
    edges = [(n, list(atoms), nb, list(bonds)) for w, n, nb, atoms, bonds in Q.edge_rows() + W.special_rows() if w == width]
    rng = random.Random(width)
    moved, origin = [], []
    for k, (n, atoms, nb, bonds) in enumerate(edges):                        # every graph row once more, renumbered
        if Q.is_graph(n, nb, bonds, width) and (n, nb) == (len(atoms), len(bonds)):
            new_atoms, new_bonds = renumbered(atoms, bonds, rng)
            moved.append((n, new_atoms, nb, new_bonds))
            origin.append(k)
    rows = edges + moved
    inputs = device_arrays(rows, width)
    R_, guard = len(rows), 64
    fills = [-0x5A5A5A5B, -0x5A5A5A5B, -0x5A5A5A5B, 0x5B5B5B5B, 0x5B]
    sizes = [R_ * width] * 3 + [R_] * 2
    out = [torch.full((size + guard,), fill, dtype=dtype, device=DEV)
           for size, fill, dtype in zip(sizes, fills, (torch.int64, torch.int32, torch.int32, torch.int32, torch.uint8))]
    lib = rt.load_library()
    with torch.cuda.device(DEV):
        rt.check(lib.mdt_mol_canon(*[rt.ptr(t) for t in inputs], width, R_, *[rt.ptr(t) for t in out], rt.current_stream()))
    torch.cuda.synchronize()
    want = [Q.canon(n, atoms, nb, bonds, width) for n, atoms, nb, bonds in rows]
    compare([t[:R_ * width].view(R_, width) for t in out[:3]] + [t[:R_] for t in out[3:]], want, width)
    assert all(bool((t[size:] == fill).all()) for t, size, fill in zip(out, sizes, fills))      # what lies after the outputs is nobody's
    flags = [r["flags"] for r in want]
    if width == 28:
        assert flags == [Q.UNDECIDED] * 2                                    # 8 atoms, every pair bonded: 40,320 leaves
    else:
        assert flags.count(Q.CANONICAL) >= 6 and (width != 8 or flags.count(0) >= 4)
    for k, r in zip(origin, want[len(edges):]):                              # defined, decided, invariant
        assert r["flags"] == want[k]["flags"] and Q.form(r) == Q.form(want[k]) and r["nodes"] == want[k]["nodes"], k
    if width == 64:
        leaves = [r["leaves"] for r in want]
        assert 128 in leaves and 2 in leaves                                 # the 64-membered ring, the 64-atom chain


def test_renumbered_rows_are_one_form_and_one_written_row(vocab):
    """24 numberings of each molecule: one relabelled graph from the op, one row from mol_write(canonical=True) -- and more than
    one row for coronene without the search."""
    rng = random.Random(5)
    molecules = SYMMETRIC + [CORONENE, DODECAHEDRANE]
    rows, owner = [], []
    for k, s in enumerate(molecules):
        _, _, atoms, bonds = K.graph(s)
        for _ in range(24):
            new_atoms, new_bonds = renumbered(atoms, bonds, rng)
            rows.append((len(atoms), new_atoms, len(bonds), new_bonds))
            owner.append(k)
    inputs = device_arrays(rows, 64)
    _, canon_atoms, canon_bonds, _, flags = torch.ops.mdt.mol_canon(*inputs)
    arrays = [t.cpu().long() for t in inputs]
    written = mol_write(*arrays, vocab, DEV, width=128, canonical=True)
    plain = mol_write(*arrays, vocab, DEV, width=128)
    torch.cuda.synchronize()
    assert flags.tolist() == [1] * len(rows) and written[3].tolist() == [1] * len(rows)
    texts, plain_texts = vocab.decode(written[0]), vocab.decode(plain[0])
    for k, s in enumerate(molecules):
        mine = [r for r in range(len(rows)) if owner[r] == k]
        want = Q.string_canon(s)
        assert {(tuple(words(canon_atoms[r:r + 1])[0]), tuple(words(canon_bonds[r:r + 1])[0])) for r in mine} == {Q.form(want)}, s
        assert len({texts[r] for r in mine}) == 1 and K.string_key(texts[mine[0]]) == K.string_key(s), s
    coronene = [r for r in range(len(rows)) if molecules[owner[r]] == CORONENE]
    assert len({plain_texts[r] for r in coronene}) > 1                      # what the search is for


def test_the_public_calls(spelled, vocab):
    strings = [s for _, sp in spelled[:60] for s in sp] + [s for s in LARGE if s not in (HEXAPHENYLBENZENE, HEXAPHENYLETHANE)] + list(C.TABLE)
    strings = [s for s in strings if len(s) <= 64]                           # (the undecided row has a test of its own)
    ids = vocab.encode(strings, 64)
    table = W.class_table(vocab.chars)
    want = [Q.string_canon(s) for s in strings]
    graphs = [C.input_arrays(s) for s in strings]
    status = [S.check(s)[0] for s in strings]
    out = mol_canon(ids.to(torch.int16), vocab, DEV)
    torch.cuda.synchronize()
    assert all(t.dtype == torch.int64 for t in out) and [tuple(t.shape) for t in out] == [(len(strings), 64)] * 3 + [(len(strings),)] * 6
    rank, canon_atoms, canon_bonds, natoms, nbonds, flags, nodes, st, _ = out
    assert rank.tolist() == [r["priority"] for r in want] and canon_atoms.tolist() == [r["canon_atoms"] for r in want]
    assert canon_bonds.tolist() == [r["canon_bonds"] for r in want] and flags.tolist() == [r["flags"] for r in want] and st.tolist() == status
    assert natoms.tolist() == [g[0] for g in graphs] and nbonds.tolist() == [g[2] for g in graphs]
    assert all(n == r["nodes"] for n, r in zip(nodes.tolist(), want) if r["flags"] == Q.CANONICAL)
    # the spellings: the search's priority where the row is decided, mdt_mol_rank's where it is not
    prio = [r["priority"] if r["flags"] == Q.CANONICAL else W.priority(*g) for r, g in zip(want, graphs)]
    written = [W.write_arrays(*g, p, table, 64) for g, p in zip(graphs, prio)]
    tokens, wflags, st, _ = mol_respell(ids, vocab, DEV, canonical=True)
    torch.cuda.synchronize()
    assert tokens.tolist() == [r["tokens"] for r in written] and wflags.tolist() == [r["flags"] for r in written] and st.tolist() == status
    for g in range(60):
        assert len({tuple(row) for row in tokens[4 * g:4 * g + 4].tolist()}) == 1, g
    lead, keep, kflags, _, _ = scaffold_keep(ids, vocab, DEV, canonical=True)
    torch.cuda.synchronize()
    maps = [C.string_scaffold(s, 1)["atom_map"] for s in strings]
    mask = [[o != 0 and m[o - 1] != 0 for o in r["token_atom"]] for r, m in zip(written, maps)]
    assert lead.tolist() == [r["tokens"] for r in written] and keep.tolist() == mask and kflags.tolist() == [r["flags"] for r in written]
    assert sum(any(m) for m in mask) >= 40
    # mol_same: every row against the next one, and against another spelling of itself
    other = ids.roll(-1, 0)
    same, undecided = mol_same(ids, other, vocab, DEV)
    again, _ = mol_same(ids, ids[:, :64].clone(), vocab, DEV)
    torch.cuda.synchronize()
    decided = [r["flags"] == Q.CANONICAL for r in want]
    nxt = want[1:] + want[:1]
    count = lambda r, g: (g[0], g[2])  # noqa: E731
    assert same.dtype == undecided.dtype == torch.bool
    assert same.tolist() == [a["flags"] == b["flags"] == Q.CANONICAL and Q.form(a) == Q.form(b) and count(a, ga) == count(b, gb)
                             for a, b, ga, gb in zip(want, nxt, graphs, graphs[1:] + graphs[:1])]
    assert not undecided.any() and again.tolist() == decided and sum(same.tolist()) >= 150 and not all(decided)


def test_an_undecided_row_in_the_public_calls(vocab):
    """hexaphenylethane: written with mdt_mol_rank's priority, and never the same as anything"""
    ids = vocab.encode([HEXAPHENYLETHANE, "CCO"], 64)
    tokens, flags, _, _ = mol_respell(ids, vocab, DEV, canonical=True)
    plain, _, _, _ = mol_respell(ids, vocab, DEV)
    same, undecided = mol_same(ids, vocab.encode(["OCC", "OCC"], 3), vocab, DEV)
    torch.cuda.synchronize()
    assert Q.string_canon(HEXAPHENYLETHANE)["flags"] == Q.UNDECIDED
    graph = C.input_arrays(HEXAPHENYLETHANE)
    want = W.write_arrays(*graph, W.priority(*graph), W.class_table(vocab.chars), 64)
    assert flags.tolist() == [1, 1] and torch.equal(tokens[0], plain[0]) and tokens[0].tolist() == want["tokens"]    # (row 1 is decided)
    assert same.tolist() == [False, True] and undecided.tolist() == [True, False]


def test_no_rows(vocab):
    none, wide = torch.zeros(0, dtype=torch.int32, device=DEV), torch.zeros(0, 64, dtype=torch.int32, device=DEV)
    out = torch.ops.mdt.mol_canon(none, wide, none, wide)
    assert [tuple(t.shape) for t in out] == [(0, 64), (0, 64), (0, 64), (0,), (0,)]
    assert rt.load_library().mdt_mol_canon(0, 0, 0, 0, 64, 0, 0, 0, 0, 0, 0, 0) == 0
    empty = torch.zeros(0, 40, dtype=torch.long)
    assert mol_canon(empty, vocab, DEV)[0].shape == (0, 40) and mol_same(empty, empty, vocab, DEV)[0].shape == (0,)
    assert mol_respell(empty, vocab, DEV, canonical=True)[0].shape == (0, 40)
