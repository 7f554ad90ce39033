"""-m gpu: mdt_mol_scaffold (csrc/k_molscaf.hip), mol_scaffold(), scaffold_key(), KnownSet.scaffold_keys(),
mdt_screen_select_classes (csrc/k_screen.hip) and the screening call with ``max_per_scaffold`` / ``novel_scaffold`` on the device.
Every comparison is exact: the counts, the atom words, the bond words, the map and the flags against the plain-int reference
tests/molscaf_ref.py (whose graphs are tests/molkey_ref.py's and whose normal forms are tests/molnorm_ref.py's), the selection
against the greedy pass restated there.  No row here can run long: two passes over the entries and at most natoms ballots a row."""
import numpy as np
import pytest
import torch

import molfp_ref as F
import molh_ref as H
import molkey_ref as K
import molnorm_ref as N
import molscaf_ref as C
import poison_util as P
import smiles_ref as S
from gpu_util import DEV, make_model
from moleculediffusiontransformer_amd import (KnownSet, NoiseSource, SmilesVocabulary, mol_scaffold, runtime as rt, scaffold_key,
                                              screen_tokens_diverse)
from moleculediffusiontransformer_amd import ops  # noqa: F401  (registers torch.ops.mdt.*)
from moleculediffusiontransformer_amd.synth import synth_normal

pytestmark = pytest.mark.gpu

ROWS_PER_BLOCK = 4                                                          # k_mol_scaffold: waves (rows) of a workgroup
NO_MOLECULE = ["", "C(", "C1CC", "C=C=C=O=C", "c1ccccc", "Xx"]
LONG = ["C" * 64, "C1CC1" + "C" * 59, "C1CC1" + "C" * 54 + "C1CC1", "C1" + "C" * 60 + "C1", "c1ccccc1" * 8, "O=C1C(=O)C(=O)C1=O"]
MASK32, MASK64 = 0xFFFFFFFF, (1 << 64) - 1
FIELDS = ("n", "atoms", "nb", "bonds", "atom_map", "flags")


@pytest.fixture(scope="module")
def pool():
    """The pool of the host test (the 2,000 random spellings, 128 mutated rows, the normal form's table) with the scaffold table,
    rows that are no molecule and the longest peels: strings of at most 64 tokens."""
    rows = [s for _, sp in K.random_spellings() for s in sp] + [s[:64] for s in S.mutated_rows(128)] + list(N.TABLE) + list(C.TABLE)
    rows += NO_MOLECULE + LONG
    assert all(len(s) <= 64 for s in rows) and sum(C.string_scaffold(s, 1)["flags"] >> 1 & 1 for s in rows) >= 1000
    return rows


@pytest.fixture(scope="module")
def vocab(pool):
    return SmilesVocabulary([None] + sorted(set(S.CHARS) | set("".join(pool)) | set("$:*%\\/csnopbBPSI")))


def graph_of(strings, vocabulary, width, normalize=False):
    """-> the four graph arrays on the device, as written or as normal forms, by the launches that come before mdt::mol_scaffold"""
    packed, n, _, _ = torch.ops.mdt.tokens_compact(vocabulary.encode(strings, width).to(DEV), 0, 1.0)
    graph = torch.ops.mdt.mol_graph(packed, n, *vocabulary.on(DEV))[:4]
    if normalize:
        hydrogens, partner, verdict, _, _ = torch.ops.mdt.mol_hydrogens(*graph, H.MAX_STEPS)
        bond_ring = torch.ops.mdt.mol_rings(*graph, hydrogens, None, None)[0]
        atoms, bonds, _ = torch.ops.mdt.mol_normalize(*graph, hydrogens, partner, verdict, bond_ring)
        graph = (graph[0], atoms, graph[2], bonds)
    return graph


def agree_arrays(got, want, what=None):
    """got: the six tensors of the op; want: the reference's rows."""
    torch.cuda.synchronize()
    natoms, atoms, nbonds, bonds, atom_map, flags = got
    assert [t.dtype for t in got] == [torch.int32] * 4 + [torch.uint8] * 2
    assert natoms.tolist() == [r["n"] for r in want] and nbonds.tolist() == [r["nb"] for r in want], what
    assert (atoms.long() & MASK32).tolist() == [r["atoms"] for r in want], what
    assert (bonds.long() & MASK32).tolist() == [r["bonds"] for r in want], what
    assert atom_map.tolist() == [r["atom_map"] for r in want] and flags.tolist() == [r["flags"] for r in want], what


def agree(strings, vocabulary, L, mode, normalize=False, what=None):
    want = [C.string_scaffold(s, mode, normalize, L) for s in strings]
    agree_arrays(torch.ops.mdt.mol_scaffold(*graph_of(strings, vocabulary, L, normalize), mode), want, what)
    return want


def unsigned(t):
    return [int(k) & MASK64 for k in t.tolist()]


@pytest.mark.parametrize("normalize", [False, True])
def test_the_whole_pool_in_all_four_modes(normalize, pool, vocab):
    graph = graph_of(pool, vocab, 64, normalize)
    for mode in C.MODES:
        want = [C.string_scaffold(s, mode, normalize) for s in pool]
        got = torch.ops.mdt.mol_scaffold(*graph, mode)
        agree_arrays(got, want, what=(mode, normalize))
        keys = unsigned(torch.ops.mdt.mol_key(*got[:4]))
        assert keys == [C.key_of(r) for r in want], mode                     # mdt::mol_key takes the scaffold arrays unchanged
        assert sum(r["flags"] == 3 for r in want) >= 800 and sum(r["flags"] == 7 for r in want) >= 100 and sum(r["flags"] == 1 for r in want) >= 500
        again = torch.ops.mdt.mol_scaffold(*got[:4], mode)                   # applying it again: the identity in modes 0, 1 and 2
        torch.cuda.synchronize()
        has = (got[5] & 2).bool()
        if mode != 3:
            assert torch.equal(again[0][has], got[0][has]) and torch.equal(again[1][has], got[1][has]) and torch.equal(again[3][has], got[3][has])
            assert (again[5][has] == 7).all() and not again[5][~has].any()
        else:
            assert (again[0][has] <= got[0][has]).all() and (again[0][has] < got[0][has]).any()    # a second pass drops X
    by = dict(zip(pool, [C.string_scaffold(s, 1, normalize) for s in pool]))
    assert by["C" * 64]["rounds"] == 32 and by["C" * 64]["flags"] == 1 and by[LONG[1]]["rounds"] == 59 and by[LONG[1]]["n"] == 3


@pytest.mark.parametrize("R_", [1, ROWS_PER_BLOCK - 1, ROWS_PER_BLOCK + 1, 67])
@pytest.mark.parametrize("L", [1, 2, 5, 32])
def test_row_shapes(L, R_, pool, vocab):
    """Molecule rows interleaved with empty rows and rows of status != 0, cut to the width (some become no molecule: a case);
    R is no multiple of the four rows of a workgroup."""
    rng = np.random.default_rng(100 * L + R_)
    small = {1: ["c", "C", "*", "", "(", "N", "F", "O"], 2: ["CC", "C=", "cc", "C", "", "C1", "N#", "OO"],
             5: ["C1CC1", "C1CO1", "CC=O", "C1CC", "", "C(C)C", "c1cc1", "C1OC1"]}
    if L in small:
        strings = [small[L][int(rng.integers(8))] for _ in range(R_)]
    else:
        strings = [["", "C(", pool[int(rng.integers(len(pool)))][:L]][min(int(rng.integers(6)), 2)] for _ in range(R_)]
    for mode in C.MODES:
        agree(strings, vocab, L, mode, what=(L, R_, mode))
    agree(strings, vocab, L, 1, normalize=True, what=(L, R_, "normal form"))


def test_no_rows_launches_nothing(vocab):
    n, rows = torch.zeros(0, dtype=torch.int32, device=DEV), torch.zeros(0, 8, dtype=torch.int32, device=DEV)
    out = torch.ops.mdt.mol_scaffold(n, rows, n, rows, 1)
    assert [tuple(t.shape) for t in out] == [(0,), (0, 8), (0,), (0, 8), (0, 8), (0,)]
    out = mol_scaffold(torch.zeros(0, 8, dtype=torch.long), vocab, DEV)
    assert out[1].shape == (0, 8) and out[5].shape == (0,)
    assert scaffold_key(torch.zeros(0, 8, dtype=torch.long), vocab, DEV, normalize=True)[0].shape == (0,)


def test_graph_arrays_that_no_scan_writes():
    """A 62-ring with an exocyclic atom and a substituent in lanes 62 and 63, a ring of all 64 lanes, entries listed twice, entries
    (x, x), the H clamp at 15, orders outside 1..4, counts outside the row, the complete graph on 8 atoms."""
    rows = [row for row in C.special_rows()]
    W = 64
    natoms = torch.tensor([row[1] for row in rows], dtype=torch.int32, device=DEV)
    nbonds = torch.tensor([row[2] for row in rows], dtype=torch.int32, device=DEV)
    atoms = torch.full((len(rows), W), 0x7FFFFFFF, dtype=torch.int32, device=DEV)    # (beyond the counts: never read)
    bonds = torch.full((len(rows), W), 0x7FFFFFFF, dtype=torch.int32, device=DEV)
    for r, (_, _, _, la, lb) in enumerate(rows):
        if la:
            atoms[r, :len(la)] = torch.tensor(la, dtype=torch.int32)
        if lb:
            words = [N.pack(e) for e in lb]
            bonds[r, :len(lb)] = torch.tensor([w - (1 << 32 if w >> 31 else 0) for w in words], dtype=torch.int32)
    for mode in C.MODES:
        want = [C.scaffold_arrays(n, la, nb, lb, mode, W) for (_, n, nb, la, lb) in rows]
        agree_arrays(torch.ops.mdt.mol_scaffold(natoms, atoms, nbonds, bonds, mode), want, what=mode)
    want = [C.scaffold_arrays(n, la, nb, lb, 1, W) for (_, n, nb, la, lb) in rows]
    assert want[0]["n"] == 63 and want[1]["n"] == 64 and want[3]["atoms"][0] >> 17 & 15 == 15 and want[6]["flags"] == 0


def test_every_output_word_is_written_over_poison(pool, vocab):
    """The entry point on outputs pre-filled by poison_util (NaN bits, then large garbage), each followed by a guard band of the same
    fill: every output word comes out defined, zero beyond the counts, and the guard comes back as it was."""
    strings = pool[::9] + NO_MOLECULE + LONG
    for L, fill, mode in ((64, P.NAN, 1), (37, P.GARBAGE, 0), (37, P.NAN, 3)):
        rows = [s[:L] for s in strings]
        inputs = graph_of(rows, vocab, L)
        R_ = len(rows)
        guard = 64                                                           # words of the fill after each output
        sizes = [(R_, torch.int32, (R_,)), (R_ * L, torch.int32, (R_, L)), (R_, torch.int32, (R_,)), (R_ * L, torch.int32, (R_, L)),
                 (R_ * L, torch.uint8, (R_, L)), (R_, torch.uint8, (R_,))]
        raw, out, before = [], [], []
        for seed, (count, dtype, shape) in enumerate(sizes):
            words = (count + 3) // 4 if dtype == torch.uint8 else count
            image = P.fill_bits(fill, words + guard, seed, DEV)
            raw.append(image)
            before.append(image.clone())
            out.append(image.view(dtype)[:count].view(shape))
        with torch.cuda.device(DEV):
            rt.check(rt.load_library().mdt_mol_scaffold(*[rt.ptr(t) for t in inputs], L, R_, mode, *[rt.ptr(t) for t in out],
                                                        rt.current_stream()))
        want = [C.string_scaffold(s, mode, False, L) for s in rows]
        agree_arrays(out, want, what=L)
        assert sum(r["flags"] == 3 for r in want) > 50 and sum(r["flags"] == 0 for r in want) >= 6 and sum(r["flags"] == 1 for r in want) > 50
        beyond_atoms = torch.arange(L, device=DEV).unsqueeze(0) >= out[0].long().unsqueeze(1)
        beyond_bonds = torch.arange(L, device=DEV).unsqueeze(0) >= out[2].long().unsqueeze(1)
        assert not out[1][beyond_atoms].any() and not out[3][beyond_bonds].any()
        for image, was, (count, dtype, _) in zip(raw, before, sizes):        # what lies after the outputs is nobody's
            nbytes = count * (1 if dtype == torch.uint8 else 4)
            assert torch.equal(image.view(torch.uint8)[nbytes:], was.view(torch.uint8)[nbytes:])


def test_the_public_calls(pool, vocab):
    rows = pool[::5] + list(C.TABLE) + NO_MOLECULE + LONG
    ids = vocab.encode(rows, 64)
    for kw, mode, normalize in ((dict(), 1, False), (dict(exocyclic=False, normalize=True), 0, True), (dict(generic=True), 3, False)):
        want = [C.string_scaffold(s, mode, normalize) for s in rows]
        out = mol_scaffold(ids.to(torch.int16), vocab, DEV, **kw)
        key, flags, status, position = scaffold_key(ids, vocab, DEV, **kw)
        torch.cuda.synchronize()
        assert all(t.dtype == torch.int64 for t in out + (key, flags, status, position))
        for name, t in zip(FIELDS, out):
            assert t.tolist() == [r[name] for r in want], (name, kw)
        assert out[6].tolist() == status.tolist() == [S.check(s)[0] for s in rows] and torch.equal(out[7], position)
        assert unsigned(key) == [C.key_of(r) for r in want] and flags.tolist() == [r["flags"] for r in want]
        known = KnownSet(ids, 64)
        got = known.scaffold_keys(vocab, DEV, **kw)
        assert unsigned(got) == sorted({C.key_of(r) for r in want} - {0}) and known.scaffold_keys(vocab, DEV, **kw) is got
    by = dict(zip(rows, unsigned(scaffold_key(ids, vocab, DEV, normalize=True)[0])))
    for s, (scaffold, _) in C.TABLE.items():                                 # the hand table, straight from the device
        assert by[s] == (N.normal_key(scaffold) if scaffold else 0), s
    assert by["Cc1ccccc1"] == by["CC(=O)c1ccccc1"] == N.normal_key("c1ccccc1") != by["O=C1CCCCC1"] != 0 == by["CCO"]


# ----------------------------------------------------------------------------------------------------------------------
# the selection
# ----------------------------------------------------------------------------------------------------------------------
SMALL = SmilesVocabulary([None] + list("CNO1()-=F"))                         # ids below 64: the distance filter takes them
MOLS = ["C1CC1C", "CC1CC1", "C1CCC1", "NC1CCC1", "C1CC1O", "O=C1CCC1", "C1CCCC1", "N1CCC1", "CCO", "CCN", "", "C(", "FC1CC1", "FC1CCC1",
        "C1COC1", "CC1COC1", "OC1CCCC1", "C1CC1C1CC1", "CCCC", "C1CC1CC", "O=C1CCC1C", "C=C1CCC1", "N1CCC1F", "OCC"]


def selection_inputs(N_, G_, seed):
    rng = np.random.default_rng(seed)
    strings = [MOLS[int(i)] for i in rng.integers(len(MOLS), size=N_ * G_)]
    ids = SMALL.encode(strings, 16).to(DEV)
    packed, length, key, _ = torch.ops.mdt.tokens_compact(ids, 0, 1.0)
    graph = torch.ops.mdt.mol_graph(packed, length, *SMALL.on(torch.device(DEV)))
    fp, count = torch.ops.mdt.mol_fp(*graph[:4], 2)
    class_key = torch.ops.mdt.mol_key(*torch.ops.mdt.mol_scaffold(*graph[:4], 1)[:4])
    score = rng.integers(0, 6, size=N_ * G_).astype(np.float32) / 4           # many ties: the lower c goes first
    score[rng.integers(N_ * G_, size=max(1, N_ * G_ // 40))] = np.nan
    return strings, score, (torch.from_numpy(score).to(DEV), key, packed, length), graph[4], fp, count, class_key


@pytest.mark.parametrize("N_,G_,K_", [(8, 5, 3), (1024, 2, 12)])
def test_screen_select_classes(N_, G_, K_):
    strings, score, head, reject, fp, count, class_key = selection_inputs(N_, G_, N_)
    classes = [C.scaffold_key(s, 1) for s in strings]
    assert unsigned(class_key) == classes and 0 in classes and len(set(classes)) >= 6
    fps = [F.string_fp(s) for s in strings]
    packed, length = head[2].cpu().numpy(), head[3].cpu().numpy()
    rj = reject.cpu().tolist()
    for most in (1, 2):
        for with_fp, sim_num, min_distance in ((False, 0, 1), (True, 49152, 1), (False, 0, 2 if N_ == 8 else 1), (True, 65536, 1)):
            got = torch.ops.mdt.screen_select_classes(*head, N_, K_, None, None, None, None, 1, min_distance, reject, fp if with_fp else None,
                                                      count if with_fp else None, sim_num, class_key, most)
            torch.cuda.synchronize()
            want = C.select_classes(score, packed, length, N_, G_, K_, classes, most, fps if with_fp else None, sim_num, min_distance, rj)
            assert (got[0].tolist(), got[1].tolist(), got[2].tolist()) == want, (most, with_fp, sim_num, min_distance)
            for g in range(G_):                                              # at most `most` kept per class; class 0 never counted
                kept = [classes[c * G_ + g] for c in want[1][g] if c >= 0]
                assert all(kept.count(k) <= most for k in set(kept) - {0})
            assert 16 in want[0] or (N_, most) == (8, 2)                    # (eight candidates seldom hold three of a class)
    # class 0 everywhere: nothing is counted; and class_key None: mdt::screen_select_similar's outputs, bit for bit
    zero = torch.zeros_like(class_key)
    for with_fp, sim_num, min_distance, r in ((False, 0, 1, None), (True, 16384, 1, reject), (False, 0, 3, reject), (True, 65536, 2, None)):
        tail = (None, None, None, None, 1, min_distance, r, fp if with_fp else None, count if with_fp else None, sim_num)
        b = torch.ops.mdt.screen_select_similar(*head, N_, K_, *tail)
        for given in (None, zero):
            a = torch.ops.mdt.screen_select_classes(*head, N_, K_, *tail, given, 1)
            torch.cuda.synchronize()
            assert all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b)), (with_fp, min_distance, given is None)


def test_screening_by_scaffold_end_to_end():
    """Two targets, six candidates each on the small model of the graph-identity test: decorated benzenes, one pyridine and an
    acyclic molecule; Kekule and aromatic spellings of one ring system.  max_per_scaffold=1 keeps one of each scaffold and gives
    bit 16 to the others; novel_scaffold=True gives bit 8 to a decoration of a known scaffold; without the keywords the result is
    today's, bit for bit."""
    G2, N2, K2, L2, T = 2, 6, 6, 32, 4
    vocab = SmilesVocabulary([None] + list("CNOcno14()-=#[H]"))
    order = [["Cc1ccccc1", "CCc1ccccc1", "CCO", "c1ccncc1", "Oc1ccccc1", "NCc1ccccc1"],
             ["CC1=CC=CC=C1", "c1ccccc1", "C1CCCCC1", "OC1CCCCC1", "CC", "O=C1CCCCC1"]]
    strings = [order[g][c] for c in range(N2) for g in range(G2)]            # row c * G + g
    tokens = vocab.encode(strings, L2)
    known = KnownSet(vocab.encode(["Nc1ccccc1", "CCCC"], L2), L2)            # aniline: the benzene scaffold is known
    fwd = make_model("cfg3")
    fwd.kernel_choice = "narrow"
    cond = synth_normal("screen/cond", (G2, 12))
    kw = dict(forward_timesteps=T, X_norm_factor=16.0, vocabulary=vocab, known_tokens=known)
    noise = lambda: NoiseSource(seed=12)   # noqa: E731
    run = lambda **more: screen_tokens_diverse(fwd, tokens, cond, DEV, N2, K2, forward_noise=noise(), **kw, **more)  # noqa: E731
    plain, off = run(), run(max_per_scaffold=None, novel_scaffold=False, scaffold_exocyclic=False, scaffold_generic=True)
    one, two, novel = run(max_per_scaffold=1), run(max_per_scaffold=2), run(novel_scaffold=True)
    normal = run(max_per_scaffold=1, normalize=True)
    both = run(max_per_scaffold=1, novel_scaffold=True, max_similarity=1.0, min_distance=2)
    torch.cuda.synchronize()
    for name in plain._fields:                                               # the defaults: today's result, field for field
        a, b = getattr(off, name), getattr(plain, name)
        assert a.dtype == b.dtype and torch.equal(a.nan_to_num(nan=-7.0), b.nan_to_num(nan=-7.0)), name
    assert not plain.status.any() and plain.count.tolist() == [N2, N2]        # all twelve are distinct molecules, none is known
    st = lambda out, g: dict(zip(order[g], out.status[:, g].tolist()))  # noqa: E731
    kept = lambda out, g: [order[g][c] for c in out.index[g].tolist() if c >= 0]  # noqa: E731
    for out, most, normalize in ((one, 1, False), (two, 2, False), (normal, 1, True)):
        for g in range(G2):                                                  # the greedy pass on the order of the plain call
            seen, want = {}, {}
            for s in kept(plain, g):
                k = C.scaffold_key(s, 1, normalize)
                want[s] = 16 if k and seen.get(k, 0) >= most else 0
                seen[k] = seen.get(k, 0) + (want[s] == 0)
            assert st(out, g) == want and kept(out, g) == [s for s in kept(plain, g) if not want[s]], (most, normalize, g)
    benzenes = [s for s in order[0] if s not in ("CCO", "c1ccncc1")]
    assert sorted(st(one, 0)[s] for s in benzenes) == [0, 16, 16, 16] and st(one, 0)["CCO"] == st(one, 0)["c1ccncc1"] == 0
    assert len(kept(one, 0)) == 3 and len(kept(two, 0)) == 4
    assert sorted(st(one, 1).values()) == [0] * 5 + [16] and st(one, 1)["O=C1CCCCC1"] == 0      # cyclohexane twice; the ketone keeps its =O
    assert st(one, 1)["CC1=CC=CC=C1"] == st(one, 1)["c1ccccc1"] == 0           # as written two scaffolds,
    assert sorted((st(normal, 1)["CC1=CC=CC=C1"], st(normal, 1)["c1ccccc1"])) == [0, 16]   # as normal forms one
    for s in order[0]:                                                       # a decoration of the known scaffold is known
        assert st(novel, 0)[s] == (8 if s in benzenes else 0), s
    assert st(novel, 1)["c1ccccc1"] == 8 and st(novel, 1)["CC1=CC=CC=C1"] == 0 and st(novel, 1)["CC"] == 0 and st(novel, 1)["C1CCCCC1"] == 0
    assert kept(novel, 0) == [s for s in kept(plain, 0) if s not in benzenes]
    assert kept(both, 0) == [s for s in kept(plain, 0) if s not in benzenes] and all(st(both, 0)[s] == 8 for s in benzenes)
