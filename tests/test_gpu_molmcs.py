"""-m gpu: mdt_mol_mcs (csrc/k_molmcs.hip), mol_mcs(), mol_difference(), mcs_tokens() and mcs_keep() on the device.  Every comparison
is exact: every size, map, bond mask, step count, graph-array word and flag against the plain-int reference tests/molmcs_ref.py
(whose graphs are tests/molkey_ref.py's), whose witness check runs on every pair as well.  No pair here can run longer than its
step cap allows: the worst one is 4,096 roots of at most 126 steps, and one capped pair of 320 roots."""
import functools
import sys

import numpy as np
import pytest
import torch

import molkey_ref as K
import molmcs_ref as C
import poison_util as P
import smiles_ref as S
from gpu_util import DEV, make_model
from moleculediffusiontransformer_amd import (NoiseSource, SmilesVocabulary, mcs_keep, mcs_tokens, mol_difference, mol_key, mol_mcs,
                                              runtime as rt)
from moleculediffusiontransformer_amd import ops  # noqa: F401  (registers torch.ops.mdt.*)
from moleculediffusiontransformer_amd.synth import synth_normal

pytestmark = pytest.mark.gpu
sys.setrecursionlimit(10000)                                                 # (the reference's walk is recursive)

# 64 tokens, 32 atoms, 31 chain bonds and 16 ring bonds that join 16 DISTINCT atom pairs (atom i with atom i + 9, then i + 7)
RING_WIDE = "".join(sym + str(d) for n, at in ((9, 0), (9, 9), (7, 18), (7, 25)) for d, sym in
                    ((d, "CCN"[(at + d - 1) % 3]) for d in range(1, n + 1)))
RING_MAX = "*" + "0123456789" + ("*" + "0123456789" * 2) * 2 + "*" + "0123456789"     # 64 tokens, 4 atoms, 30 ring bonds
CAP_A = "C(C)(C)(C)C(C)(C)C(C)(C)C(C)(C)C(C)(C)C(C)(C)C"
CAP_B = "CC(C)C(C)C(C)C(C)C(C)C(C)C(C)C"
ROWS_PER_BLOCK = 2                                                           # k_mol_mcs: waves (pairs in flight) of a workgroup
MASK64 = (1 << 64) - 1
NAMES = ("size", "map_a", "bond_a", "steps", "out_natoms", "out_atoms", "out_nbonds", "out_bonds", "atom_map", "flags")


@pytest.fixture(scope="module")
def spelled():
    return K.random_spellings(graphs=60)


@pytest.fixture(scope="module")
def vocab(spelled):
    chars = set(S.CHARS) | set("".join(s for _, sp in spelled for s in sp)) | set("$:*%\\/")
    return SmilesVocabulary([None] + sorted(chars))


@pytest.fixture(scope="module")
def pool(spelled):
    """Spellings of random graphs, small hand strings, and broken rows that are no molecule."""
    rng = np.random.default_rng(5)
    broken = [s[:int(rng.integers(1, len(s) + 1))] + ("(" if r % 3 else "") for r, s in enumerate(S.mutated_rows(24)) if s]
    hand = ["C1CC1C", "CC(C)(C)C", "C12CC1C2", "C.CO", "[NH3+]CC[O-]", "NCCO", "c1ccccc1O", "C1=CC=CC=C1", "CC(=O)Nc1ccccc1", "C", "*C*", ""]
    return [s for _, sp in spelled for s in sp[:2]] + broken + hand


@functools.lru_cache(maxsize=None)
def reference(a, b, mode, LA, LB):
    """One pair of strings -> the reference's words in NAMES' order; the witness is checked on the way"""
    w = C.string_mcs(a, b, mode, LA, LB)
    (aa, ab), (ba, bb) = C.graph_of(a), C.graph_of(b)
    C.check_witness(w, aa, ab, ba, bb, mode)
    return (w["size"], tuple(w["map_a"]), w["bond_a"], w["steps"], w["out_natoms"], tuple(w["out_atoms"]), w["out_nbonds"],
            tuple(w["out_bonds"]), tuple(w["atom_map"]), w["flags"])


def graph_arrays(strings, vocabulary, width):
    """The graph arrays of mdt::mol_graph, int32 on the device; a string that is no molecule has no atoms."""
    packed, n, _, _ = torch.ops.mdt.tokens_compact(vocabulary.encode(strings, width).to(DEV), 0, 1.0)
    return torch.ops.mdt.mol_graph(packed, n, *vocabulary.on(DEV))[:4]


def words(got):
    """The ten outputs of mdt::mol_mcs -> per row a tuple in NAMES' order, unsigned"""
    size, map_a, bond_a, steps, natoms, atoms, nbonds, bonds, atom_map, flags = [t.cpu() for t in got]
    return [(tuple(size[r].tolist()), tuple(map_a[r].tolist()), int(bond_a[r]) & MASK64, int(steps[r]), int(natoms[r]),
             tuple(int(x) & 0xFFFFFFFF for x in atoms[r].tolist()), int(nbonds[r]), tuple(bonds[r].tolist()), tuple(atom_map[r].tolist()),
             int(flags[r])) for r in range(size.shape[0])]


def compare(got, a_strings, b_strings, mode, LA, LB, what=None):
    R_ = len(a_strings)
    assert [(t.dtype, tuple(t.shape)) for t in got] == [
        (torch.int32, (R_, 2)), (torch.uint8, (R_, LA)), (torch.int64, (R_,)), (torch.int32, (R_,)), (torch.int32, (R_,)),
        (torch.int32, (R_, LA)), (torch.int32, (R_,)), (torch.int32, (R_, LA)), (torch.uint8, (R_, LA)), (torch.uint8, (R_,))]
    want = [reference(a, b_strings[r if len(b_strings) > 1 else 0], mode, LA, LB) for r, a in enumerate(a_strings)]
    for r, (g, w) in enumerate(zip(words(got), want)):
        for name, x, y in zip(NAMES, g, w):
            assert x == y, (what, r, a_strings[r], name, x, y)
    return want


def agree(a_strings, b_strings, vocabulary, LA, LB, mode=0, what=None):
    got = torch.ops.mdt.mol_mcs(*graph_arrays(a_strings, vocabulary, LA), *graph_arrays(b_strings, vocabulary, LB), mode)
    torch.cuda.synchronize()
    return compare(got, a_strings, b_strings, mode, LA, LB, what)


@pytest.mark.parametrize("widths, R_", [((1, 1), 1), ((1, 1), 2 * ROWS_PER_BLOCK + 1), ((33, 64), 1), ((33, 64), 4 * ROWS_PER_BLOCK - 1),
                                        ((64, 20), 2 * ROWS_PER_BLOCK + 1), ((64, 20), 41), ((21, 21), 4 * ROWS_PER_BLOCK - 1)])
def test_mol_mcs_row_shapes(widths, R_, pool, vocab):
    """R = 1, one more and one less than a multiple of the waves per workgroup, LA != LB, LA = LB = 1, both modes"""
    LA, LB = widths
    rng = np.random.default_rng(1000 * LA + R_)
    a = [pool[int(rng.integers(len(pool)))][:LA] for _ in range(R_)]
    b = [pool[int(rng.integers(len(pool)))][:LB] for _ in range(R_)]
    want = agree(a, b, vocab, LA, LB, mode=(R_ + LA) % 2, what=(LA, LB, R_))
    assert R_ < 40 or (any(w[9] & C.COMMON for w in want) and any(w[9] == 0 for w in want))


def test_full_width_rows_the_cap_and_rows_that_are_no_molecule(vocab):
    """RING_MAX names each of its three atom pairs eleven times.  A's entries count each for itself and B is read as a set, so the
    bound of step 2 (3 bonds) lies under the floor the greedy descent reaches (33) and every root returns at once: the definition's
    answer for such a row -- one that mdt_mol_write calls not writable -- is (0, 1), and that is what is compared here."""
    a = ["*" * 64, RING_MAX, CAP_A, "C12C3C4C1C5C2C3C45", "", "C(", "CCO", "c1ccccc1c1ccccc1", "C1CC1C", "C1CC1", RING_WIDE]
    b = ["*" * 64, RING_MAX, CAP_B, "C12C3C4C1C5C2C3C45", "CCO", "CCO", "C(", "c1ccccc1Cc1ccccc1", "CC(C)(C)C", "CCC", RING_WIDE]
    assert len(RING_WIDE) == 64 and len(C.graph_of(RING_WIDE)[0]) == 32 and len(set(map(frozenset, (e[:2] for e in C.graph_of(RING_WIDE)[1])))) == 47
    assert len(RING_MAX) == 64 and all(len(s) <= 64 for s in a + b)
    want = agree(a, b, vocab, 64, 64, what="full width")
    assert want[0][0] == (63, 64) and want[0][3] == 8002 and want[0][9] == C.PAIR | C.COMMON | C.WHOLE_A | C.WHOLE_B
    assert want[1][0] == (0, 1) and want[1][9] == C.PAIR | C.COMMON
    assert want[2][9] & C.UNDECIDED and want[2][0] == (13, 14)              # the capped pair: its lower bound, and the flag
    assert want[3][0] == (12, 8) and want[3][9] == C.PAIR | C.COMMON | C.WHOLE_A | C.WHOLE_B
    assert all(w[9] == 0 and w[0] == (0, 0) and w[3] == 0 for w in want[4:7])
    assert want[8][0] == (3, 4) and want[9][0] == (2, 3)
    # the full-width row whose closures join distinct pairs: the walk at 47 entries and 584 roots finds all of it
    assert want[10][0] == (47, 32) and want[10][3] == 1260 and want[10][9] == C.PAIR | C.COMMON | C.WHOLE_A | C.WHOLE_B
    exact = agree(a[:2] + a[3:], b[:2] + b[3:], vocab, 64, 64, mode=1, what="full width, exact")
    assert exact[0][0] == (63, 64)


def test_one_b_row_for_every_a_row(pool, vocab):
    a = pool[::3] + ["", "C("]
    for target, LB in (("CC(=O)Nc1ccccc1", 64), ("C(", 9), ("N", 1)):
        want = agree(a, [target], vocab, 64, LB, what=("RB = 1", target))
        assert (target == "C(") == all(w[9] == 0 for w in want)
    with pytest.raises(RuntimeError, match="rows"):
        torch.ops.mdt.mol_mcs(*graph_arrays(a[:4], vocab, 64), *graph_arrays(a[:3], vocab, 64), 0)


def test_the_same_pair_gives_the_same_words_anywhere_and_twice(pool, vocab):
    """A pair at another row index and in another batch, and the whole call again, bit for bit"""
    a, b = pool[:37], pool[5:42]
    ga, gb = graph_arrays(a, vocab, 64), graph_arrays(b, vocab, 64)
    first = torch.ops.mdt.mol_mcs(*ga, *gb, 0)
    again = torch.ops.mdt.mol_mcs(*ga, *gb, 0)
    order = list(np.random.default_rng(3).permutation(37))
    moved = agree([a[i] for i in order] + [CAP_A, "C1CC1"], [b[i] for i in order] + [CAP_B, "CCC"], vocab, 64, 64, what="moved")
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(first, again))
    rows = words(first)
    assert [moved[k] for k in range(37)] == [rows[i] for i in order]


def test_graph_arrays_that_no_scan_writes_and_no_rows(vocab):
    c, n = K.descriptor("C"), K.descriptor("N")
    odd = [(3, 2, [(0, 3, 1), (1, 2, 1)]), (9, 0, []), (2, 9, []), (-1, 0, []), (2, -1, []), (2, 2, [(0, 1, 1)] * 2), (2, 1, [(0, 0, 2)]),
           (2, 1, [(0, 1, 7)]), (2, 2, [(1, 1, 2), (1, 0, 1)]), (3, 2, [(0, 1, 1), (2, 1, 1)]), (1, 0, []), (4, 3, [(0, 1, 1), (0, 2, 1), (0, 3, 1)]),
           (3, 4, [(0, 1, 1), (1, 0, 1), (1, 2, 2), (2, 1, 1)]), (0, 0, [])]
    pairs = [(i, j) for i in range(len(odd)) for j in range(len(odd))]
    word_of = [c, c, n, c, c, c, c, c]
    def side(index):
        natoms = torch.tensor([odd[i][0] for i in index], dtype=torch.int32, device=DEV)
        nbonds = torch.tensor([odd[i][1] for i in index], dtype=torch.int32, device=DEV)
        atoms = torch.tensor([word_of] * len(index), dtype=torch.int32, device=DEV)
        bonds = torch.zeros(len(index), 8, dtype=torch.int32)
        for r, i in enumerate(index):
            for e, (x, y, o) in enumerate(odd[i][2]):
                bonds[r, e] = x | y << 8 | o << 16
        return natoms, atoms, nbonds, bonds.to(DEV)
    got = torch.ops.mdt.mol_mcs(*side([i for i, _ in pairs]), *side([j for _, j in pairs]), 0)
    torch.cuda.synchronize()
    want = []
    for i, j in pairs:
        (na, nba, ea), (nb, nbb, eb) = odd[i], odd[j]
        w = C.mcs_arrays(na, word_of, nba, ea, nb, word_of, nbb, eb, 0, 8, 8)
        if w["flags"]:
            C.check_witness(w, word_of[:na], ea[:nba], word_of[:nb], eb[:nbb])
        want.append((w["size"], tuple(w["map_a"]), w["bond_a"], w["steps"], w["out_natoms"], tuple(w["out_atoms"]), w["out_nbonds"],
                     tuple(w["out_bonds"]), tuple(w["atom_map"]), w["flags"]))
    assert words(got) == want
    at = {p: k for k, p in enumerate(pairs)}
    assert all(want[at[(i, j)]][9] == 0 for i in (0, 1, 2, 3, 4, 13) for j in range(len(odd)))
    # an entry listed twice counts twice on A's side; against ONE such bond of B the bound (1) lies under the floor (2): the limit the
    # header states for rows that name a pair of atoms twice
    assert want[at[(5, 12)]][0] == (2, 2) and want[at[(12, 5)]][0] == (0, 1)
    assert want[at[(6, 6)]][0] == (0, 1) and want[at[(7, 7)]][0] == (0, 1)    # (a, a) and order 7 join nothing
    a4 = side([5, 6])
    empty = torch.ops.mdt.mol_mcs(*[t[:0] for t in a4], *[t[:0] for t in a4], 0)
    assert [tuple(t.shape) for t in empty] == [(0, 2), (0, 8), (0,), (0,), (0,), (0, 8), (0,), (0, 8), (0, 8), (0,)]


def test_every_output_word_is_written_over_poison(pool, vocab):
    """The entry point on outputs pre-filled with garbage, with NaN bits and with zeros, each followed by a guard band of the same
    fill: the three results are identical and the reference's, and the guard comes back as it was."""
    a = [s[:37] for s in pool[::5]] + ["", "C(", "C" * 37, "C1CC1C"]
    b = [pool[(7 * k + 3) % len(pool)][:23] for k in range(len(a) - 4)] + ["CC", "CC", "C(", "CC(C)(C)C"]
    LA, LB, R_ = 37, 23, len(a)
    assert len(b) == R_
    inputs = graph_arrays(a, vocab, LA) + graph_arrays(b, vocab, LB)
    sizes = [(R_ * 2, torch.int32), (R_ * LA, torch.uint8), (R_, torch.int64), (R_, torch.int32), (R_, torch.int32),
             (R_ * LA, torch.int32), (R_, torch.int32), (R_ * LA, torch.int32), (R_ * LA, torch.uint8), (R_, torch.uint8)]
    shapes = [(R_, 2), (R_, LA), (R_,), (R_,), (R_,), (R_, LA), (R_,), (R_, LA), (R_, LA), (R_,)]
    results = []
    for fill in (P.GARBAGE, P.NAN, P.ZERO):
        raw, before, out, guard = [], [], [], 64
        for seed, ((count, dtype), shape) in enumerate(zip(sizes, shapes)):
            nbytes = count * torch.empty(0, dtype=dtype).element_size()
            image = P.fill_bits(fill, (nbytes + 7) // 8 * 2 + guard, seed, DEV)
            raw.append(image)
            before.append(image.clone())
            out.append(image.view(torch.uint8)[:nbytes].view(dtype).view(shape))
        lib = rt.load_library()
        with torch.cuda.device(DEV):
            rt.check(lib.mdt_mol_mcs(*[rt.ptr(t) for t in inputs[:4]], LA, R_, *[rt.ptr(t) for t in inputs[4:]], LB, R_, 0,
                                     *[rt.ptr(t) for t in out], rt.current_stream()))
        torch.cuda.synchronize()
        compare(out, a, b, 0, LA, LB, fill)
        for image, was, (count, dtype) in zip(raw, before, sizes):           # what lies after the outputs is nobody's
            nbytes = count * torch.empty(0, dtype=dtype).element_size()
            assert torch.equal(image.view(torch.uint8)[nbytes:], was.view(torch.uint8)[nbytes:]), fill
        results.append([t.clone() for t in out])
    assert all(torch.equal(x, y) for other in results[1:] for x, y in zip(results[0], other))
    assert results[0][9].any() and not results[0][9].all()


def test_the_python_surface_end_to_end(pool, vocab):
    a = pool[:30] + ["CC(=O)Nc1ccccc1", "C1=CC=CC=C1C", "", "C1CC1C", CAP_A, "[NH3+]CC[O-]"]
    b = pool[7:37] + ["CC(=O)Oc1ccccc1", "c1ccccc1C", "CC", "CC(C)(C)C", CAP_B, "NCCO"]
    for atoms in ("element", "exact"):
        mode = 1 if atoms == "exact" else 0
        if mode:                                                             # (the capped pair once is enough)
            a, b = a[:34] + a[35:], b[:34] + b[35:]
        ia, ib = vocab.encode(a, 64), vocab.encode(b, 64)
        r = mol_mcs(ia, ib, vocab, DEV, atoms=atoms)
        torch.cuda.synchronize()
        want = [reference(x, y, mode, 64, 64) for x, y in zip(a, b)]
        assert mode or (want[35][0] == (3, 4) and r.undecided[34])
        assert r.bonds.tolist() == [w[0][0] for w in want] and r.atoms.tolist() == [w[0][1] for w in want]
        assert r.map_a.tolist() == [list(w[1]) for w in want] and r.in_a.tolist() == [[v != 0 for v in w[1]] for w in want]
        assert r.in_b.tolist() == [[t + 1 in w[1] for t in range(64)] for w in want]
        assert r.undecided.tolist() == [bool(w[9] & C.UNDECIDED) for w in want] and r.steps.tolist() == [w[3] for w in want]
        assert r.whole_a.tolist() == [bool(w[9] & C.WHOLE_A) for w in want] and r.whole_b.tolist() == [bool(w[9] & C.WHOLE_B) for w in want]
        assert r.pair.tolist() == [bool(w[9] & C.PAIR) for w in want]
        assert r.natoms.tolist() == [w[4] for w in want] and r.graph_atoms.tolist() == [list(w[5]) for w in want]
        assert r.nbonds.tolist() == [w[6] for w in want] and r.graph_bonds.tolist() == [list(w[7]) for w in want]
        assert r.atom_map.tolist() == [list(w[8]) for w in want]
        sims = []
        for x, y, w in zip(a, b, want):
            (aa, ab), (ba, bb) = C.graph_of(x), C.graph_of(y)
            sims.append(C.similarity(dict(flags=w[9], size=w[0]), aa, ab, ba, bb))
        assert r.similarity.dtype == torch.float64 and r.similarity.tolist() == sims
        assert r.a_status.tolist() == [S.check(s)[0] for s in a] and r.b_status.tolist() == [S.check(s)[0] for s in b]
        only_a, only_b, undecided = mol_difference(ia, ib, vocab, DEV, atoms=atoms)
        na, nb = [len(C.graph_of(s)[0]) for s in a], [len(C.graph_of(s)[0]) for s in b]
        assert only_a.tolist() == [[bool(w[9] & C.PAIR) and x < n and w[1][x] == 0 for x in range(64)] for w, n in zip(want, na)]
        assert only_b.tolist() == [[bool(w[9] & C.PAIR) and t < n and t + 1 not in w[1] for t in range(64)] for w, n in zip(want, nb)]
        assert torch.equal(undecided, r.undecided)
    assert want[34][0] == (1, 2) and not r.pair[32]                          # exact: the charged ends stay out
    # the normal form finds the benzene ring that the Kekule spelling hides
    plain = mol_mcs(vocab.encode(["C1=CC=CC=C1C"], 64), vocab.encode(["c1ccccc1C"], 64), vocab, DEV)
    normal = mol_mcs(vocab.encode(["C1=CC=CC=C1C"], 64), vocab.encode(["c1ccccc1C"], 64), vocab, DEV, normalize=True)
    assert plain.atoms.tolist() == [1] and normal.atoms.tolist() == [7] and normal.whole_a.all() and normal.similarity.tolist() == [1.0]
    # mcs_tokens(): the written row reads back to the key of the graph arrays
    r = mol_mcs(ia, ib, vocab, DEV)                                          # (the rows of the exact pass)
    for canonical in (False, True):
        tokens, flags, undecided, _, _ = mcs_tokens(ia, ib, vocab, DEV, canonical=canonical)
        key_arrays = torch.ops.mdt.mol_key(r.natoms.int(), r.graph_atoms.int(), r.nbonds.int(), r.graph_bonds.int())
        key_read, status, _ = mol_key(tokens, vocab, DEV)
        torch.cuda.synchronize()
        written = flags == 1
        assert tokens.shape == (len(a), 64) and torch.equal(written, r.atoms > 0) and int(written.sum()) >= 25
        assert torch.equal(key_read[written], key_arrays[written]) and not status[written].any() and not tokens[~written].any()
    one = mcs_tokens(vocab.encode(["CC(=O)Nc1ccccc1"], 64), vocab.encode(["CC(=O)Oc1ccccc1"], 64), vocab, DEV, width=20)[0]
    assert one.shape == (1, 20) and sorted(vocab.decode(one)[0]) == sorted("c1ccccc1")


def test_refining_a_lead_around_what_it_shares_with_another_molecule():
    """mcs_keep()'s mask fed to refine_keep_tokens() on the tiny model: every kept position of the output is the lead's id"""
    m = make_model("tiny")                                                   # 16 ids, rows of 32 positions
    vocab = SmilesVocabulary([None] + list("CNOcno1()-=#[H]"))
    leads = ["CC(=O)Nc1ccccc1", "OC(=O)CCN", "OCC", "NC1CC1C(=O)O", "C(", "O=C1CCC1CN", "C1=CC=CC=C1C(=O)N"]
    others = ["CC(=O)Oc1ccccc1", "NCCC(=O)OC", "N", "C1CC1", "CC", "C(", "c1ccccc1C(N)=O"]
    assert len(vocab) == 15 == m.pred_dim - 1 and m.max_length == 32
    tokens, keep, complete, flags, status, _ = mcs_keep(vocab.encode(leads, 32), vocab.encode(others, 32), vocab, DEV)
    torch.cuda.synchronize()
    assert flags.tolist() == [1, 1, 1, 1, 0, 1, 1] and complete.all() and not keep[4].any() and not keep[2].any() and not keep[5].any()
    for r, (lead, other) in enumerate(zip(leads, others)):
        want = C.string_mcs(lead, other)
        text = vocab.decode(tokens)[r]
        atoms_kept = sum(1 for ch, k in zip(text, keep[r].tolist()) if k and ch in "CNOcno")
        assert atoms_kept == want["size"][1], (lead, other, text)
    seq = synth_normal("molmcs/seq", (len(leads), 12))
    for start in (2, [0, 5, 3, 1, 4, 2, 6]):
        out = m.refine_keep_tokens(seq, DEV, tokens.cpu(), start_step=start, cond_scale=2.0, timesteps=8, noise=NoiseSource(seed=17),
                                   keep_mask=keep.cpu())
        torch.cuda.synchronize()
        assert out.shape == tokens.shape and torch.equal(out[keep], tokens[keep]) and int(keep.sum()) >= 12
    one = mcs_keep(vocab.encode(leads, 32), vocab.encode(["c1ccccc1"], 32), vocab, DEV, normalize=True)
    assert one[1][0].any() and one[1][6].any() and not one[1][1].any()       # one row for every lead; benzene through the normal form
