"""-m gpu: mdt_mol_fp, mdt_fp_tanimoto_rows, mdt_fp_nearest (csrc/k_molfp.hip) and mdt_screen_select_similar (csrc/k_screen.hip),
KnownSet.fingerprints and the screening call with the two similarity thresholds on the device.  Every comparison is exact: bits,
counts and indices against the plain-int reference tests/molfp_ref.py (whose graphs are tests/molkey_ref.py's)."""
import numpy as np
import pytest
import torch

import molfp_ref as F
import molkey_ref as K
import smiles_ref as S
from gpu_util import DEV, make_model
from moleculediffusiontransformer_amd import (KnownSet, NoiseSource, SmilesVocabulary, mol_fingerprint, nearest_known_tanimoto,
                                              screen_tokens_diverse, tanimoto)
from moleculediffusiontransformer_amd import ops  # noqa: F401  (registers torch.ops.mdt.*)
from moleculediffusiontransformer_amd import runtime as rt
from moleculediffusiontransformer_amd.synth import synth_normal

pytestmark = pytest.mark.gpu

CHUNK = rt.FP_KNOWN_CHUNK
RING_SYSTEM = "C1C2C3C4C5C6C7C8C9C%10C%11C%12C%13C%14C%15C1C2C3"              # (as the graph key's full-width test)
RING_MAX = "*" + "0123456789" + ("*" + "0123456789" * 2) * 2 + "*" + "0123456789"     # 64 tokens, 4 atoms, 30 ring bonds


@pytest.fixture(scope="module")
def spelled():
    return K.random_spellings()


@pytest.fixture(scope="module")
def vocab(spelled):
    chars = set(S.CHARS) | set("".join(s for _, sp in spelled for s in sp)) | set("$:*%\\/")
    return SmilesVocabulary([None] + sorted(chars))


@pytest.fixture(scope="module")
def pool(spelled):
    """Strings of at most 64 tokens: every spelling, and mutated rows of which most are no molecule."""
    rng = np.random.default_rng(5)
    broken = [s[:int(rng.integers(1, len(s) + 1))] + ("(" if r % 3 else "") for r, s in enumerate(S.mutated_rows(768)) if s]
    assert sum(F.string_fp(s) == 0 for s in broken) > 0.5 * len(broken)
    return [s for _, sp in spelled for s in sp] + broken


def to_dev(fps):
    """Python-int fingerprints -> int64 (R, 16) on the device."""
    a = np.array([F.words(f) for f in fps], dtype=np.uint64).reshape(len(fps), 16)
    return torch.from_numpy(a.view(np.int64)).to(DEV)


def agree(strings, vocabulary, L, radius=2, ids=None, what=None):
    ids = vocabulary.encode(strings, L) if ids is None else ids
    fp, count, status, _ = mol_fingerprint(ids, vocabulary, DEV, radius)
    torch.cuda.synchronize()
    assert fp.dtype == count.dtype == torch.int64 and fp.shape == (len(strings), 16) and count.shape == (len(strings),)
    got = fp.cpu().numpy().view(np.uint64)
    for r, s in enumerate(strings):
        want = F.string_fp(s, radius)
        assert (got[r].tolist(), int(count[r])) == (F.words(want), F.popcount(want)), (what, r, s)
        assert (want == 0) == (int(status[r]) != 0 or s == ""), (what, r, s)
    return got


@pytest.mark.parametrize("R_", [1, 63, 64, 65, 257])                       # a workgroup of mdt_mol_fp takes 4 rows, of the graph 64
@pytest.mark.parametrize("L", [1, 33, 64])
def test_mol_fp_shapes(L, R_, pool, vocab):
    rng = np.random.default_rng(100 * L + R_)
    strings = [pool[int(rng.integers(len(pool)))][:L] for _ in range(R_)]
    agree(strings, vocab, L, radius=int(rng.integers(4)), what=(L, R_))


def test_mol_fp_full_width_rows_every_radius_and_rows_that_are_no_molecule(vocab, pool):
    chain = "C" * 64
    assert len(RING_MAX) == 64 and S.check(RING_MAX) == (S.OK, -1) and [len(x) for x in K.graph(RING_MAX)[2:]] == [4, 33]
    strings = [chain, RING_MAX, RING_SYSTEM, "C1" * 32, "c1ccccc1" * 8, "[13CH4]" * 9, "", "C(", "C" * 63 + "("] + \
        [s for pair in K.EQUAL_PAIRS + K.DIFFERENT_PAIRS for s in pair]
    for radius in range(4):
        got = agree(strings, vocab, 64, radius, what=radius)
        assert got[0].any() and not got[6].any() and not got[7].any() and not got[8].any()
    by = dict(zip(strings, map(tuple, got)))
    for a, b in K.EQUAL_PAIRS:
        assert by[a] == by[b], (a, b)
    broken = [s for s in pool if F.string_fp(s) == 0][:300] + pool[:100]    # mostly no molecule
    agree(broken, vocab, 64, what="broken")
    # graph arrays no scan writes: counts outside [0, L], a bond that names an atom the row does not have -> no fingerprint
    c = K.descriptor("C")
    natoms = torch.tensor([3, 9, 2, -1, 2, 2, 2], dtype=torch.int32, device=DEV)
    nbonds = torch.tensor([2, 0, 9, 0, -1, 2, 1], dtype=torch.int32, device=DEV)
    atoms = torch.full((7, 8), c, dtype=torch.int32, device=DEV)
    bonds = torch.zeros(7, 8, dtype=torch.int32, device=DEV)
    bonds[0, :2] = torch.tensor([0 | 3 << 8 | 1 << 16, 1 | 2 << 8 | 1 << 16])
    bonds[5, :2] = 0 | 1 << 8 | 1 << 16                                      # a bond listed twice counts twice
    bonds[6, 0] = 0 | 0 << 8 | 2 << 16                                       # a bond of an atom to itself: twice at that atom
    fp, count = torch.ops.mdt.mol_fp(natoms, atoms, nbonds, bonds, 3)
    torch.cuda.synchronize()
    want = [0] * 5 + [F.fingerprint([c, c], [(0, 1, 1)] * 2, 3, 8), F.fingerprint([c, c], [(0, 0, 2)], 3, 8)]
    assert fp.cpu().numpy().view(np.uint64).tolist() == [F.words(w) for w in want] and want[5] and want[6]
    assert count.tolist() == [F.popcount(w) for w in want]
    # a 63-bond ring system at full width (a string of 64 tokens cannot spell it: a ring bond costs two tokens): two fused rings
    # over atoms 0..61 with a nitrogen, a double bond and a bridge, and two atoms on their own
    n_, o_ = K.descriptor("N"), K.descriptor("O")
    ring_atoms = [c] * 64
    ring_atoms[17], ring_atoms[63] = n_, o_
    ring_bonds = [(a, (a + 1) % 62, 2 if a == 40 else 1) for a in range(62)] + [(0, 31, 1)]
    assert len(ring_bonds) == 63
    words = [a | b << 8 | o << 16 for a, b, o in ring_bonds] + [0]
    for radius in range(4):
        fp, count = torch.ops.mdt.mol_fp(torch.tensor([64], dtype=torch.int32, device=DEV),
                                         torch.tensor([ring_atoms], dtype=torch.int32, device=DEV),
                                         torch.tensor([63], dtype=torch.int32, device=DEV),
                                         torch.tensor([words], dtype=torch.int32, device=DEV), radius)
        want = F.fingerprint(ring_atoms, ring_bonds, radius)
        assert fp.cpu().numpy().view(np.uint64).tolist() == [F.words(want)] and count.tolist() == [F.popcount(want)] and want


def test_mol_fp_with_zeros_scattered_through_a_row(vocab):
    rng = np.random.default_rng(7)
    strings = [s for s, _, _ in S.TABLES] + [s for pair in K.EQUAL_PAIRS for s in pair]
    ids = vocab.encode(strings, 32).numpy()
    spread = np.zeros((len(strings), 64), np.int64)
    for r, s in enumerate(strings):
        spread[r, np.sort(rng.choice(64, len(s), replace=False))] = ids[r, :len(s)]
    for dtype in (torch.int64, torch.int16):
        agree(strings, vocab, 64, ids=torch.from_numpy(spread).to(dtype), what=dtype)


def test_tanimoto_rows(pool, vocab):
    rng = np.random.default_rng(3)
    a = [pool[int(i)] for i in rng.integers(len(pool), size=300)] + [p[0] for p in K.EQUAL_PAIRS + K.DIFFERENT_PAIRS] + ["", "CCO", ""]
    b = [pool[int(i)] for i in rng.integers(len(pool), size=300)] + [p[1] for p in K.EQUAL_PAIRS + K.DIFFERENT_PAIRS] + ["CCO", "C(", ""]
    b[:100] = a[:100][::-1]
    sim, inter, union = tanimoto(vocab.encode(a, 64), vocab.encode(b, 64), vocab, DEV)
    torch.cuda.synchronize()
    want = [F.counts(F.string_fp(x), F.string_fp(y)) for x, y in zip(a, b)]
    assert inter.tolist() == [w[0] for w in want] and union.tolist() == [w[1] for w in want]
    assert sim.dtype == torch.float32 and torch.equal(sim.cpu(), inter.cpu().float() / union.cpu().clamp(min=1).float())
    n = len(K.EQUAL_PAIRS)
    assert all(i == u > 0 for i, u in want[300:300 + n]) and sim[-3:].tolist() == [0.0, 0.0, 0.0]
    assert sum(0 < i < u for i, u in want) > 100                             # fractions strictly between 0 and 1 are compared too


@pytest.fixture(scope="module")
def known_fps(pool):
    """2 * CHUNK + 1 fingerprints with repeats (respellings) and zeros (rows that are no molecule)."""
    rng = np.random.default_rng(11)
    return [F.string_fp(pool[int(i)]) for i in rng.integers(len(pool), size=2 * CHUNK + 1)]


@pytest.mark.parametrize("R_", [1, 64, 65])
def test_fp_nearest(R_, pool, known_fps):
    rng = np.random.default_rng(R_)
    queries = [F.string_fp(pool[int(i)]) for i in rng.integers(len(pool), size=R_)]
    q = to_dev(queries)
    for M_ in (1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1):
        index, inter, union = torch.ops.mdt.fp_nearest(q, to_dev(known_fps[:M_]))
        torch.cuda.synchronize()
        want = [F.nearest(f, known_fps[:M_]) for f in queries]
        assert list(zip(index.tolist(), inter.tolist(), union.tolist())) == want, (R_, M_)
    assert len({w[0] for w in want}) > 1 or R_ == 1


def test_fp_nearest_ties(vocab):
    # the same molecule respelled at known indices 5 and CHUNK + 200, fingerprints from the device: index 5 wins
    filler = ["N" * (1 + k % 30) + "O" * (1 + k // 30) for k in range(CHUNK + 300)]
    filler[5], filler[CHUNK + 200] = "C1CC1C", "CC1CC1"
    known_fp = mol_fingerprint(vocab.encode(filler, 64), vocab, DEV)[0]
    query_fp = mol_fingerprint(vocab.encode(["C1(C)CC1", "C("], 64), vocab, DEV)[0]
    index, inter, union = torch.ops.mdt.fp_nearest(query_fp, known_fp)
    torch.cuda.synchronize()
    assert index.tolist() == [5, 0] and inter[0] == union[0] > 0 and inter[1] == 0
    assert F.nearest(F.string_fp("C1(C)CC1"), [F.string_fp(s) for s in filler])[0] == 5
    # through the public call: KnownSet sorts its rows by key, index is a row of KnownSet.packed
    known = KnownSet(vocab.encode(filler, 64), 64)
    spelt = vocab.decode(known.packed)
    fps = [F.string_fp(x) for x in spelt]
    lo, hi = sorted((spelt.index("C1CC1C"), spelt.index("CC1CC1")))
    sim, index, inter, union = nearest_known_tanimoto(vocab.encode(["C1(C)CC1", "C(", "NNO"], 64), known, vocab, DEV)
    torch.cuda.synchronize()
    want = [F.nearest(F.string_fp(x), fps) for x in ("C1(C)CC1", "C(", "NNO")]
    assert list(zip(index.tolist(), inter.tolist(), union.tolist())) == want and index[0] == lo < hi and sim.tolist()[:2] == [1.0, 0.0]
    fp, count = known.fingerprints(vocab, DEV)                               # all rows of packed, in that order
    assert fp.cpu().numpy().view(np.uint64).tolist() == [F.words(f) for f in fps] and count.tolist() == [F.popcount(f) for f in fps]
    assert known.fingerprints(vocab, DEV)[0] is fp
    # hand-made words: equal fractions from different counts, in different chunks -- the lower index wins either way round
    q, half, two_quarters, nothing = 0b11, 0b01, 0b1111, 1 << 900
    assert F.counts(q, half) == (1, 2) and F.counts(q, two_quarters) == (2, 4) and F.counts(q, nothing)[0] == 0
    for low, high in ((two_quarters, half), (half, two_quarters)):
        hand = [nothing] * (2 * CHUNK + 1)
        hand[9], hand[2 * CHUNK] = low, high
        index, inter, union = torch.ops.mdt.fp_nearest(to_dev([q]), to_dev(hand))
        torch.cuda.synchronize()
        assert (int(index[0]), int(inter[0]), int(union[0])) == (9,) + F.counts(q, low) == F.nearest(q, hand)
    hand[9] = 0b0101                                                         # 1/3 at the low index: now the high one wins
    index, inter, union = torch.ops.mdt.fp_nearest(to_dev([q]), to_dev(hand))
    assert (int(index[0]), int(inter[0]), int(union[0])) == (2 * CHUNK, 2, 4) == F.nearest(q, hand)
    # an all-zero query, and a known set whose rows are all zero: similarity 0, the lowest index
    index, inter, union = torch.ops.mdt.fp_nearest(to_dev([0, q]), to_dev(hand))
    assert (int(index[0]), int(inter[0]), int(union[0])) == (0, 0, 1) == F.nearest(0, hand)
    index, inter, union = torch.ops.mdt.fp_nearest(to_dev([0, q]), to_dev([0] * (CHUNK + 3)))
    torch.cuda.synchronize()
    assert index.tolist() == [0, 0] and inter.tolist() == [0, 0] and union.tolist() == [0, 2]


# ----------------------------------------------------------------------------------------------------------------------
# the selection
# ----------------------------------------------------------------------------------------------------------------------
SMALL = SmilesVocabulary([None] + list("CNO1()-=F"))                         # ids below 64: the distance filter takes them
MOLS = ["CCO", "OCC", "C(O)C", "C-C-O", "C1CC1C", "CC1CC1", "C1(C)CC1", "CCN", "NCC", "CC=O", "C=CO", "CCCC", "CC(C)C", "C(C)CC",
        "CCOC", "COCC", "FC(F)F", "C(", "", "CCCCO", "OCCCC", "CC(=O)O", "OC(C)=O", "NC(=O)C"]


def selection_inputs(N, G_, seed):
    rng = np.random.default_rng(seed)
    strings = [MOLS[int(i)] for i in rng.integers(len(MOLS), size=N * G_)]
    ids = SMALL.encode(strings, 16).to(DEV)
    packed, length, key, _ = torch.ops.mdt.tokens_compact(ids, 0, 1.0)
    graph = torch.ops.mdt.mol_graph(packed, length, *SMALL.on(torch.device(DEV)))
    fp, count = torch.ops.mdt.mol_fp(*graph[:4], 2)
    score = rng.integers(0, 6, size=N * G_).astype(np.float32) / 4            # many ties: the lower c goes first
    score[rng.integers(N * G_, size=max(1, N * G_ // 40))] = np.nan
    reject = graph[4]                                                        # the check's status: 32 / 64, never kept
    rows = [SMALL.encode([s], 16)[0, :len(s)].tolist() for s in strings]
    return strings, rows, score, (torch.from_numpy(score).to(DEV), key, packed, length), reject, fp, count


@pytest.mark.parametrize("N", [1, 2, 257])
def test_screen_select_similar(N):
    G_ = 3
    strings, rows, score, head, reject, fp, count = selection_inputs(N, G_, N)
    fps = [F.string_fp(s) for s in strings]
    extra = torch.from_numpy(np.random.default_rng(N).integers(0, 2, size=N * G_).astype(np.uint8) * 8).to(DEV) | reject   # reject bits set
    for K_ in sorted({1, N}):
        for sim_num, min_distance, rj in ((65536, 1, reject), (1, 1, reject), (16384, 1, reject), (19661, 3, reject), (65536, 3, extra),
                                          (6554, 1, None)):
            status, index, cnt = torch.ops.mdt.screen_select_similar(*head, N, K_, None, None, None, None, 1, min_distance, rj, fp, count,
                                                                     sim_num)
            torch.cuda.synchronize()
            want = F.select_similar(score.tolist(), rows, fps, N, G_, K_, sim_num, min_distance, None if rj is None else rj.cpu().tolist())
            assert (status.tolist(), index.tolist(), cnt.tolist()) == want, (N, K_, sim_num, min_distance)
            st = np.array(want[0]).reshape(N, G_)
            if sim_num == 65536 and min_distance == 1:                       # a threshold of 1.0 passes over only identical fingerprints
                for g in range(G_):
                    kept = [fps[c * G_ + g] for c in want[1][g] if c >= 0]
                    assert all(fps[c * G_ + g] in kept for c in range(N) if st[c, g] == 16)
                    assert K_ < N or len(set(kept)) == len(kept) == len({fps[c * G_ + g] for c in range(N) if st[c, g] in (0, 16)})
            if sim_num == 1 and K_ == N:                                     # a low threshold keeps one candidate per group of overlapping ones
                for g in range(G_):
                    kept = [fps[c * G_ + g] for c in want[1][g] if c >= 0]
                    assert all(F.counts(a, b)[0] == 0 for i, a in enumerate(kept) for b in kept[:i])
        # without fingerprints: the selection that ran before, bit for bit on the same inputs
        for min_distance, rj in ((1, None), (3, reject), (2, extra)):
            a = torch.ops.mdt.screen_select_similar(*head, N, K_, None, None, None, None, 1, min_distance, rj, None, None, 0)
            b = torch.ops.mdt.screen_select_diverse_reject(*head, N, K_, None, None, None, None, 1, min_distance, rj)
            torch.cuda.synchronize()
            assert all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b)), (N, K_, min_distance)
            want = F.select_similar(score.tolist(), rows, None, N, G_, K_, 0, min_distance, None if rj is None else rj.cpu().tolist())
            assert (a[0].tolist(), a[1].tolist(), a[2].tolist()) == want


def test_screening_by_similarity_end_to_end():
    """Two targets, eight candidates each on the small model of the graph-identity test.  The known set holds ethanol (spelled a
    fourth way) and butane: every ethanol is known at threshold 1.0 whatever its spelling; of the rest, one that is at least 0.2
    similar to a better kept one is passed over.  The reference chain: the order of the eligible candidates from the same call without
    the thresholds (keep = N), the fingerprints and the greedy pass of tests/molfp_ref.py."""
    G2, N2, K2, L2, T = 2, 8, 3, 32, 4
    vocab = SmilesVocabulary([None] + list("CNO1()-="))
    order = [["CCO", "C1CC1C", "OCC", "C(", "CC1CC1", "CCCCN", "NCCCC", "CC=O"],
             ["CC1CC1", "CCN", "C-C-O", "NCC", "C(", "C1(C)CC1", "CCCC=O", "C(O)C"]]
    strings = [order[g][c] for c in range(N2) for g in range(G2)]            # row c * G + g
    tokens = vocab.encode(strings, L2)
    known = KnownSet(vocab.encode(["C(C)O", "CCCC"], L2), L2)
    fwd = make_model("cfg3")
    fwd.kernel_choice = "narrow"
    cond = synth_normal("screen/cond", (G2, 12))
    kw = dict(forward_timesteps=T, X_norm_factor=16.0, known_tokens=known, vocabulary=vocab)
    noise = lambda: NoiseSource(seed=12)   # noqa: E731
    out = screen_tokens_diverse(fwd, tokens, cond, DEV, N2, K2, max_similarity=0.2, max_known_similarity=1.0, forward_noise=noise(), **kw)
    plain = screen_tokens_diverse(fwd, tokens, cond, DEV, N2, N2, forward_noise=noise(), **kw)
    none = screen_tokens_diverse(fwd, tokens, cond, DEV, N2, N2, max_similarity=None, max_known_similarity=None, forward_noise=noise(), **kw)
    torch.cuda.synchronize()
    for name in plain._fields:                                               # both at None: today's result, field for field
        a, b = getattr(none, name), getattr(plain, name)
        assert a.dtype == b.dtype and torch.equal(a.nan_to_num(nan=-7.0), b.nan_to_num(nan=-7.0)), name
    assert plain.status.cpu().numpy().reshape(-1).tolist() == [32 if s == "C(" else 0 for s in strings]
    fps = [F.string_fp(s) for s in strings]
    known_fps = [F.string_fp(s) for s in vocab.decode(known.packed)]
    want = plain.status.cpu().numpy().copy()                                 # (N, G)
    index, count = [], []
    for g in range(G2):
        kept = []
        for c in plain.index[g].tolist():                                    # the eligible candidates in (score, c) order
            if c < 0:
                continue
            r = c * G2 + g
            _, inter, union = F.nearest(fps[r], known_fps)
            if F.at_least(inter, union, 65536):
                want[c, g] |= 8
            elif any(F.at_least(*F.counts(fps[r], fps[o * G2 + g]), 13107) for o in kept):
                want[c, g] |= 16
            elif len(kept) < K2:
                kept.append(c)
        index.append(kept + [-1] * (K2 - len(kept)))
        count.append(len(kept))
    assert out.status.dtype == torch.uint8 and np.array_equal(out.status.cpu().numpy(), want)
    assert out.index.tolist() == index and out.count.tolist() == count
    ethanol = {"CCO", "OCC", "C-C-O", "C(O)C"}
    assert all((want.reshape(-1)[r] == 8) == (s in ethanol) for r, s in enumerate(strings))
    assert (want == 16).sum() >= 2 and min(count) >= 1                        # the respelled ring is passed over in both groups
