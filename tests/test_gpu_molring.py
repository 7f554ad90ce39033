"""-m gpu: mdt_mol_rings (csrc/k_molring.hip), mol_rings(), mol_descriptors() and the screening call with ``limits`` on the device.
Every comparison is exact: bond_ring, atom_ring, the sixteen descriptors and the flags against the plain-int reference
tests/molring_ref.py (whose graphs are tests/molkey_ref.py's and whose hydrogens are tests/molh_ref.py's).  No row here can run long:
at most nbonds searches of at most natoms levels a row."""
import random

import numpy as np
import pytest
import torch

import molh_ref as H
import molkey_ref as K
import molring_ref as R
import poison_util as P
import smiles_ref as S
from gpu_util import DEV, make_model
from moleculediffusiontransformer_amd import (DESCRIPTOR_NAMES, DescriptorLimits, NoiseSource, SmilesVocabulary, mol_descriptors, mol_rings,
                                              runtime as rt, screen_tokens_diverse)
from moleculediffusiontransformer_amd import ops  # noqa: F401  (registers torch.ops.mdt.*)
from moleculediffusiontransformer_amd.synth import synth_normal

pytestmark = pytest.mark.gpu

ROWS_PER_BLOCK = 4                                                          # k_mol_rings: waves (rows) of a workgroup
NO_MOLECULE = ["", "C(", "C1CC", "C=C=C=O=C", "c1ccccc", "Xx"]
FUSED_64 = "C%10CCC(CC%10)C%11CCC(CC%11)C%12CCC(CC%12)C%13CCC(CC%13)C1CCCCC1"         # 64 tokens, five rings in a row
LADDER = "C1C2C3" + "C" * 20 + "C3C2C1"                                               # nested closures: a 22-ring inside two 4-rings


@pytest.fixture(scope="module")
def pool():
    """Strings of at most 64 tokens: the table, random spellings, rows that are no molecule, mutated rows."""
    rows = list(R.TABLE) + [s for _, sp in K.random_spellings()[:120] for s in sp] + NO_MOLECULE
    rows += [s[:64] for s in S.mutated_rows(128)]
    assert all(len(s) <= 64 for s in rows) and sum(R.string_rings(s)["desc"][5] > 0 for s in rows) > 100
    return rows


@pytest.fixture(scope="module")
def vocab(pool):
    return SmilesVocabulary([None] + sorted(set(S.CHARS) | set("".join(pool)) | set("$:*%\\/csnopbBPSI")))


def graph_arrays(strings, vocabulary, width):
    """-> (natoms, atoms, nbonds, bonds, hydrogens) on the device, by the two launches that come before mdt::mol_rings"""
    packed, n, _, _ = torch.ops.mdt.tokens_compact(vocabulary.encode(strings, width).to(DEV), 0, 1.0)
    graph = torch.ops.mdt.mol_graph(packed, n, *vocabulary.on(DEV))[:4]
    return (*graph, torch.ops.mdt.mol_hydrogens(*graph, H.MAX_STEPS)[0])


def agree_arrays(got, want, flags=None, what=None):
    """got: the four tensors of the op; want: the reference's rows; flags: the expected flags (None: all zero)."""
    torch.cuda.synchronize()
    bond_ring, atom_ring, desc, got_flags = got
    assert (bond_ring.dtype, atom_ring.dtype, desc.dtype, got_flags.dtype) == (torch.uint8, torch.uint8, torch.int32, torch.uint8)
    assert bond_ring.tolist() == [r["bond_ring"] for r in want], what
    assert atom_ring.tolist() == [r["atom_ring"] for r in want], what
    assert desc.tolist() == [r["desc"] for r in want], what
    assert got_flags.tolist() == (flags if flags is not None else [0] * len(want)), what


def agree(strings, vocabulary, L, limits=None, what=None):
    want = [R.string_rings(s, L) for s in strings]
    lo, hi = (None, None) if limits is None else limits.on(DEV)
    flags = None if limits is None else [R.flag(r["desc"], r["molecule"], limits.lo.tolist(), limits.hi.tolist()) for r in want]
    agree_arrays(torch.ops.mdt.mol_rings(*graph_arrays(strings, vocabulary, L), lo, hi), want, flags, what)
    return want


def test_the_table_and_the_spelling_pool_through_the_op_and_the_public_calls(pool, vocab):
    want = agree(pool, vocab, 64, what="pool")
    agree(pool, vocab, 64, limits=DescriptorLimits(max_rings=1, max_weight=150.0, min_heavy_atoms=2), what="pool, bounded")
    ids = vocab.encode(pool, 64)
    atom_ring, bond_ring, desc, verdict, status, position = mol_rings(ids, vocab, DEV)
    desc2, verdict2, status2, position2 = mol_descriptors(ids.to(torch.int16), vocab, DEV)
    torch.cuda.synchronize()
    assert all(t.dtype == torch.int64 for t in (atom_ring, bond_ring, desc, verdict, status, position, desc2, verdict2))
    assert atom_ring.tolist() == [r["atom_ring"] for r in want] and bond_ring.tolist() == [r["bond_ring"] for r in want]
    assert desc.tolist() == desc2.tolist() == [r["desc"] for r in want]
    assert verdict.tolist() == verdict2.tolist() == [H.string_hydrogens(s)["verdict"] for s in pool]
    assert status.tolist() == status2.tolist() == [S.check(s)[0] for s in pool] and torch.equal(position, position2)
    by = {s: dict(zip(DESCRIPTOR_NAMES, row)) for s, row in zip(pool, desc.tolist())}
    assert by["c1ccc2ccccc2c1"]["rings"] == 2 and by["c1ccc2ccccc2c1"]["largest_ring"] == 6 and by["C12C3C4C1C5C2C3C45"]["rings"] == 5
    assert by["cc"]["aromatic_outside_ring"] == 2 and by["CCCC"]["rotatable_bonds"] == 1 and by["CC(=O)NC"]["weight"] == 73095
    assert by[R.WIDEST_RING]["smallest_ring"] == 62 and not any(by["C("].values())
    for s, (ring_of_bond, ring_of_atom, named) in R.TABLE.items():           # the hand table, straight from the device
        row = pool.index(s)
        assert bond_ring[row, :len(ring_of_bond)].tolist() == ring_of_bond and atom_ring[row, :len(ring_of_atom)].tolist() == ring_of_atom
        assert {k: by[s][k] for k in named} == named, s


@pytest.mark.parametrize("R_", [1, ROWS_PER_BLOCK - 1, ROWS_PER_BLOCK, ROWS_PER_BLOCK + 1, 67])
@pytest.mark.parametrize("L", [1, 33, 64])
def test_row_shapes(L, R_, pool, vocab):
    """Molecule rows interleaved with empty rows and rows of status != 0, cut to the width (some become no molecule: a case)."""
    rng = np.random.default_rng(100 * L + R_)
    if L == 1:
        strings = [["c", "C", "*", "", "(", "N", "F", "O"][int(rng.integers(8))] for _ in range(R_)]
    else:
        strings = [["", "C(", pool[int(rng.integers(len(pool)))][:L]][min(int(rng.integers(6)), 2)] for _ in range(R_)]
    agree(strings, vocab, L, what=(L, R_))
    agree(strings, vocab, L, limits=DescriptorLimits(max_ring_atoms=5, min_carbons=1), what=(L, R_, "bounded"))


def test_no_rows_launches_nothing(vocab):
    n, rows, h = (torch.zeros(0, dtype=torch.int32, device=DEV), torch.zeros(0, 8, dtype=torch.int32, device=DEV),
                  torch.zeros(0, 8, dtype=torch.uint8, device=DEV))
    out = torch.ops.mdt.mol_rings(n, rows, n, rows, h, None, None)
    assert [tuple(t.shape) for t in out] == [(0, 8), (0, 8), (0, 16), (0,)]
    out = torch.ops.mdt.mol_rings(n, rows, n, rows, h, *DescriptorLimits(max_rings=0).on(DEV))
    assert [tuple(t.shape) for t in out] == [(0, 8), (0, 8), (0, 16), (0,)]
    assert mol_rings(torch.zeros(0, 8, dtype=torch.long), vocab, DEV)[2].shape == (0, 16)


def test_full_width_rows(vocab):
    strings = [R.WIDEST_RING, "C" * 64, "c" * 64, FUSED_64, "c1ccccc1" * 8, "*" * 64, "", "C(", LADDER, LADDER.replace("C", "c"),
               "[nH]1cccc1" * 6 + "cccc", "C1CC1" * 12 + "CCCC", "N" * 63 + "O"]
    assert len(R.WIDEST_RING) == len(FUSED_64) == 64 and all(len(s) <= 64 for s in strings)
    want = agree(strings, vocab, 64, what="full width")
    named = [dict(zip(R.NAMES, r["desc"])) for r in want]
    assert want[0]["bond_ring"][:62] == [62] * 62 and want[0]["atom_ring"][:62] == [62] * 62 and named[0]["largest_ring"] == 62
    assert named[1]["rotatable_bonds"] == 61 and named[1]["rings"] == 0 and named[2]["aromatic_outside_ring"] == 64
    assert named[3]["rings"] == 5 and named[3]["rotatable_bonds"] == 4 and named[4]["rings"] == 8 and named[5]["hetero_atoms"] == 64
    assert named[8]["rings"] == 3 and named[8]["largest_ring"] == 22 and named[8]["smallest_ring"] == 4 and named[12]["acceptors"] == 64


def test_graph_arrays_that_no_scan_writes():
    """A duplicated entry is one edge; an entry (a, a) is none; an order 0 or 7 is an edge like any other; counts outside [0, L] and
    a bond naming an atom >= natoms give all-zero outputs and flag 0, under bounds nothing can meet."""
    c, n_, h = K.descriptor("C"), K.descriptor("N"), K.descriptor("H", True)
    k8 = [(i, j, 1) for i in range(8) for j in range(i)]
    odd = [(3, [c] * 3, 2, [(0, 3, 1), (1, 2, 1)], [0] * 3), (29, [c] * 28, 0, [], [0] * 28), (2, [c] * 2, 29, [], [0] * 2), (-1, [], 0, [], []),
           (2, [c] * 2, -1, [], [0] * 2), (0, [], 0, [], []),
           (3, [c] * 3, 4, [(0, 1, 1), (1, 0, 1), (1, 2, 1), (2, 0, 1)], [2] * 3), (3, [c] * 3, 3, [(0, 0, 1), (0, 1, 1), (1, 2, 3)], [1, 2, 3]),
           (2, [c] * 2, 1, [(0, 1, 7)], [0, 0]), (4, [c, n_, c, c], 4, [(0, 1, 0), (1, 2, 65535), (2, 3, 1), (3, 0, 1)], [255, 255, 0, 1]),
           (2, [c] * 2, 2, [(0, 1, 1)] * 2, [3, 3]), (4, [h, n_, h, c], 3, [(0, 1, 1), (1, 2, 1), (1, 3, 1)], [0, 0, 0, 3]),
           (1, [c], 1, [(0, 0, 1)], [4]), (8, [c] * 8, 28, k8, [0] * 8),
           (28, [c] * 28, 28, [(i, (i + 1) % 28, 1) for i in range(28)], [2] * 28)]
    W = 28
    natoms = torch.tensor([n for n, _, _, _, _ in odd], dtype=torch.int32, device=DEV)
    nbonds = torch.tensor([nb for _, _, nb, _, _ in odd], dtype=torch.int32, device=DEV)
    atoms = torch.full((len(odd), W), 0x7FFFFFFF, dtype=torch.int32, device=DEV)    # (beyond the counts: never read)
    bonds = torch.full((len(odd), W), 0x7FFFFFFF, dtype=torch.int32, device=DEV)
    hydrogens = torch.full((len(odd), W), 0xA5, dtype=torch.uint8, device=DEV)
    for r, (_, listed_atoms, _, listed, listed_h) in enumerate(odd):
        if listed_atoms:
            atoms[r, :len(listed_atoms)] = torch.tensor(listed_atoms, dtype=torch.int32)
            hydrogens[r, :len(listed_h)] = torch.tensor(listed_h, dtype=torch.uint8)
        for e, (a, b, o) in enumerate(listed):
            word = a | b << 8 | o << 16
            bonds[r, e] = word - (1 << 32 if word >> 31 else 0)              # (the uint32 bits in int32 storage)
    want = [R.rings_arrays(n, list(la), nb, list(lb), list(lh), W) for n, la, nb, lb, lh in odd]
    never = DescriptorLimits(min_rings=5, max_rings=4)                       # bounds no row can meet
    got = torch.ops.mdt.mol_rings(natoms, atoms, nbonds, bonds, hydrogens, *never.on(DEV))
    agree_arrays(got, want, flags=[0] * 6 + [128] * (len(odd) - 6))
    assert all(not any(r["bond_ring"] + r["atom_ring"] + r["desc"]) for r in want[:6])
    named = [dict(zip(R.NAMES, r["desc"])) for r in want]
    assert want[6]["bond_ring"][:4] == [3] * 4 and named[6]["rings"] == 1 and want[7]["bond_ring"][:3] == [0] * 3
    assert want[9]["bond_ring"][:4] == [4] * 4 and named[9]["donors"] == 1 and named[9]["weight"] == 3 * 12011 + 14007 + 511 * 1008
    assert named[10]["rings"] == 0 and named[11]["heavy_atoms"] == 2 and named[11]["weight"] == 2 * 1008 + 14007 + 12011 + 3 * 1008
    assert want[13]["bond_ring"][:28] == [3] * 28 and named[13]["rings"] == 21 and want[14]["bond_ring"] == [28] * 28
    agree_arrays(torch.ops.mdt.mol_rings(natoms, atoms, nbonds, bonds, hydrogens, None, None), want)


def test_flags_against_bounds_that_each_reject_one_known_row(vocab):
    strings = ["CCO", "C1CC1", "c1ccccc1", "CCCCCC", "C.C", "CC(=O)NC", "C(", ""]
    graph = graph_arrays(strings, vocab, 16)
    want = [R.string_rings(s, 16) for s in strings]
    for bounds, rejected in ((dict(max_components=1), "C.C"), (dict(max_largest_ring=5), "c1ccccc1"), (dict(max_aromatic_atoms=0), "c1ccccc1"),
                             (dict(max_rotatable_bonds=2), "CCCCCC"), (dict(max_weight=86.177), "CCCCCC"), (dict(max_weight=86.178), None),
                             (dict(max_hetero_atoms=1), "CC(=O)NC"), (dict(min_heavy_atoms=3), "C.C"), (dict(min_sp3_carbons=1), "c1ccccc1"),
                             (dict(max_smallest_ring=5, max_donors=1, min_carbons=2), "c1ccccc1"), (dict(max_ring_bonds=5, min_weight=30.0), "c1ccccc1"),
                             (dict(min_ring_atoms=0, max_ring_atoms=3, max_acceptors=2), "c1ccccc1"), (dict(), None)):
        limits = DescriptorLimits(**bounds)
        flags = [R.flag(r["desc"], r["molecule"], limits.lo.tolist(), limits.hi.tolist()) for r in want]
        assert flags == [128 if s == rejected else 0 for s in strings], bounds
        agree_arrays(torch.ops.mdt.mol_rings(*graph, *limits.on(DEV)), want, flags, what=bounds)
    agree_arrays(torch.ops.mdt.mol_rings(*graph, None, None), want, what="no bounds")
    natoms, atoms, nbonds, bonds, hydrogens = graph                          # flags == NULL: nothing is written, the rest is
    out = [torch.zeros(8, 16, dtype=torch.uint8, device=DEV), torch.zeros(8, 16, dtype=torch.uint8, device=DEV),
           torch.zeros(8, 16, dtype=torch.int32, device=DEV)]
    lo, hi = DescriptorLimits(max_rings=0).on(DEV)
    with torch.cuda.device(DEV):
        rt.check(rt.load_library().mdt_mol_rings(rt.ptr(natoms), rt.ptr(atoms), rt.ptr(nbonds), rt.ptr(bonds), rt.ptr(hydrogens), 16, 8,
                                                 rt.ptr(lo), rt.ptr(hi), *[rt.ptr(t) for t in out], 0, rt.current_stream()))
    agree_arrays((*out, torch.zeros(8, dtype=torch.uint8, device=DEV)), want, what="flags NULL")


def test_every_output_word_is_written_over_poison(pool, vocab):
    """The entry point on outputs pre-filled by poison_util (NaN bits, then large garbage), each followed by a guard band of the same
    fill: every output word comes out defined, zero beyond the counts, and the guard comes back as it was."""
    strings = pool[::3] + ["", "C(", R.WIDEST_RING, FUSED_64]
    limits = DescriptorLimits(max_rings=1)
    for L, fill in ((64, P.NAN), (37, P.GARBAGE)):
        rows = [s[:L] for s in strings]
        natoms, atoms, nbonds, bonds, hydrogens = graph_arrays(rows, vocab, L)
        R_ = len(rows)
        guard = 64                                                           # words of the fill after each output
        sizes = [(R_ * L, torch.uint8, (R_, L)), (R_ * L, torch.uint8, (R_, L)), (R_ * 16, torch.int32, (R_, 16)), (R_, torch.uint8, (R_,))]
        raw, out, before = [], [], []
        for seed, (count, dtype, shape) in enumerate(sizes):
            words = (count + 3) // 4 if dtype == torch.uint8 else count
            image = P.fill_bits(fill, words + guard, seed, DEV)
            raw.append(image)
            before.append(image.clone())
            out.append(image.view(dtype)[:count].view(shape))
        with torch.cuda.device(DEV):
            rt.check(rt.load_library().mdt_mol_rings(rt.ptr(natoms), rt.ptr(atoms), rt.ptr(nbonds), rt.ptr(bonds), rt.ptr(hydrogens), L, R_,
                                                     *[rt.ptr(t) for t in limits.on(DEV)], *[rt.ptr(t) for t in out], rt.current_stream()))
        want = [R.string_rings(s, L) for s in rows]
        flags = [R.flag(r["desc"], r["molecule"], limits.lo.tolist(), limits.hi.tolist()) for r in want]
        agree_arrays(out, want, flags, what=L)
        assert 0 < sum(f != 0 for f in flags) < len(flags)
        beyond_atoms = torch.arange(L, device=DEV).unsqueeze(0) >= natoms.long().unsqueeze(1)
        beyond_bonds = torch.arange(L, device=DEV).unsqueeze(0) >= nbonds.long().unsqueeze(1)
        assert not out[0][beyond_bonds].any() and not out[1][beyond_atoms].any()
        for image, was, (count, dtype, _) in zip(raw, before, sizes):        # what lies after the outputs is nobody's
            nbytes = count * (1 if dtype == torch.uint8 else 4)
            assert torch.equal(image.view(torch.uint8)[nbytes:], was.view(torch.uint8)[nbytes:])


def test_the_same_call_twice_gives_identical_bits(pool, vocab):
    graph = graph_arrays(pool, vocab, 64)
    lo, hi = DescriptorLimits.lipinski().on(DEV)
    first = torch.ops.mdt.mol_rings(*graph, lo, hi)
    second = torch.ops.mdt.mol_rings(*graph, lo, hi)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, second))


def test_screening_with_limits_end_to_end():
    """Three targets, six candidates each on the small model of the graph-identity test.  Under max_rings=0 no ring-bearing
    candidate is kept and each carries bit 128; limits=None returns what the call returns without the keyword, bit for bit."""
    G2, N2, K2, L2, T = 3, 6, 3, 32, 4
    vocab = SmilesVocabulary([None] + list("CNOcno1()-=#[H]"))
    order = [["C1CC1", "CCO", "c1ccccc1", "CC(=O)N", "C1CCCCC1O", "CC"],
             ["CCN", "c1cc[nH]c1", "C(", "CC(C)C", "C1=CC=CC=C1", "OCCO"],
             ["CC#N", "cc", "C1CC1C1CC1", "O", "N1CCCC1", "CCCC"]]
    strings = [order[g][c] for c in range(N2) for g in range(G2)]            # row c * G + g
    tokens = vocab.encode(strings, L2)
    fwd = make_model("cfg3")
    fwd.kernel_choice = "narrow"
    cond = synth_normal("screen/cond", (G2, 12))
    kw = dict(forward_timesteps=T, X_norm_factor=16.0, vocabulary=vocab)
    noise = lambda: NoiseSource(seed=12)   # noqa: E731
    limits = DescriptorLimits(max_rings=0)
    out = screen_tokens_diverse(fwd, tokens, cond, DEV, N2, K2, limits=limits, forward_noise=noise(), **kw)
    again = screen_tokens_diverse(fwd, tokens, cond, DEV, N2, K2, limits=limits, forward_noise=noise(), **kw)
    plain = screen_tokens_diverse(fwd, tokens, cond, DEV, N2, N2, forward_noise=noise(), **kw)
    off = screen_tokens_diverse(fwd, tokens, cond, DEV, N2, N2, limits=None, forward_noise=noise(), **kw)
    both = screen_tokens_diverse(fwd, tokens, cond, DEV, N2, K2, limits=limits, kekulize=True, forward_noise=noise(), **kw)
    torch.cuda.synchronize()
    for name in plain._fields:                                               # None: today's result, field for field; and repeatable
        for a, b in ((getattr(off, name), getattr(plain, name)), (getattr(again, name), getattr(out, name)), (getattr(both, name), getattr(out, name))):
            assert a.dtype == b.dtype and torch.equal(a.nan_to_num(nan=-7.0), b.nan_to_num(nan=-7.0)), name
    ringed = np.array([128 if R.string_rings(s)["desc"][5] > 0 else 0 for s in strings], dtype=np.uint8).reshape(N2, G2)
    assert ringed[:, 0].tolist() == [128, 0, 128, 0, 128, 0] and ringed[:, 1].tolist() == [0, 128, 0, 0, 128, 0]
    assert ringed[:, 2].tolist() == [0, 0, 128, 0, 128, 0]
    assert all(H.string_hydrogens(s)["verdict"] == 0 for s in strings)       # (so kekulize=True adds nothing above)
    assert not (plain.status.cpu().numpy()[ringed != 0] & 128).any()         # without limits nothing carries the bit
    want = plain.status.cpu().numpy() | ringed
    assert out.status.dtype == torch.uint8 and np.array_equal(out.status.cpu().numpy(), want)
    index = [[c for c in plain.index[g].tolist() if c >= 0 and not ringed[c, g]][:K2] for g in range(G2)]
    assert out.index.tolist() == [kept + [-1] * (K2 - len(kept)) for kept in index] and out.count.tolist() == [len(k) for k in index]
    assert all(want[c, g] & 128 == 0 for g in range(G2) for c in index[g]) and sum(len(k) for k in index) > 0
    kept = [strings[c * G2 + g] for g in range(G2) for c in index[g]]
    assert all(R.string_rings(s)["desc"][5] == 0 for s in kept)              # no ring-bearing candidate is kept


def test_random_rows_keep_their_answer_when_respelled(vocab):
    rng = random.Random(7)
    groups = [sp for _, sp in K.random_spellings()[120:160]]
    rng.shuffle(groups)
    strings = [s for sp in groups for s in sp]
    desc = mol_descriptors(vocab.encode(strings, 64), vocab, DEV)[0].tolist()
    at = 0
    for sp in groups:
        assert all(desc[at + k] == desc[at] == R.string_rings(sp[0])["desc"] for k in range(len(sp))), sp
        at += len(sp)
