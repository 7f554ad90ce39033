"""-m gpu: the edit-distance kernels (csrc/k_edit.hip), mdt_screen_select_diverse (csrc/k_screen.hip) and the public functions on
the device.  Every comparison is of integers and exact, against the numpy reference tests/edit_ref.py; the end-to-end runs are
compared with sample_tokens -> predict_properties_from_tokens -> that reference on the host, bit for bit under a pinned
kernel_choice."""
import numpy as np
import pytest
import torch

from gpu_util import DEV, make_model
import edit_ref as E
import screen_ref as R
from moleculediffusiontransformer_amd import (KnownSet, NoiseSource, edit_distance, nearest_known, predict_properties_from_tokens,
                                              screen_candidates, screen_tokens_diverse)
from moleculediffusiontransformer_amd import ops  # noqa: F401  (registers torch.ops.mdt.*)
from moleculediffusiontransformer_amd import runtime as rt
from moleculediffusiontransformer_amd.synth import synth_normal

pytestmark = pytest.mark.gpu

CHUNK = rt.EDIT_KNOWN_CHUNK


def dev(a, dtype=torch.int32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def pack(rows, L):
    """Lists of ids -> (packed int32 (R, L), length int32 (R))."""
    packed, length = np.zeros((len(rows), L), np.int32), np.zeros(len(rows), np.int32)
    for r, row in enumerate(rows):
        packed[r, :len(row)], length[r] = row, len(row)
    return packed, length


# ----------------------------------------------------------------------------------------------------------------------
# mdt::edit_distance
# ----------------------------------------------------------------------------------------------------------------------
def dev_distance(a, la, b, lb):
    return torch.ops.mdt.edit_distance(dev(a), dev(la), dev(b), dev(lb)).cpu().numpy()


def planted_pairs(rng, L):
    """The edges of the recurrence at width L: empty sides, equal rows, a FULL row against itself with one substitution at either
    end and against itself shifted by one, rows over one symbol."""
    full = rng.integers(1, 64, L).tolist()
    other = lambda t: t % 63 + 1                                               # another id in [1, 64)
    some = rng.integers(1, 64, max(1, L // 2)).tolist()
    return [([], []), ([], some), (some, []), ([], full), (full, []), (full, full), (some, some),
            (full, [other(full[0])] + full[1:]), (full, full[:-1] + [other(full[-1])]),
            (full, full[1:] + [other(full[0])]), (full, full[1:]),
            ([63] * L, [63] * (L // 2)), ([7] * (L // 3), [7] * L), ([63] * L, [62] * L)]


@pytest.mark.parametrize("R_", [1, 5, 67])                                     # 67: no multiple of a wave
@pytest.mark.parametrize("L", [1, 2, 63, 64])                                  # 64: the probe bit is bit 63; nothing shifts by 64
def test_edit_distance_matches_the_reference(L, R_):
    rng = np.random.default_rng(100 * L + R_)
    raw_a = rng.integers(1, 64, (R_, L)) * (rng.random((R_, L)) > 0.4)        # ids in [1, 64), id 63 among them; ~40 % zeros
    raw_b = np.where(rng.random((R_, L)) < 0.7, raw_a, rng.integers(0, 64, (R_, L)))     # b: a with about a third redrawn
    raw_a[0, 0] = 63
    a, la, _, _ = R.compact(raw_a)
    b, lb, _, _ = R.compact(raw_b)
    pa, pb = zip(*planted_pairs(rng, L))
    for (a, la), (b, lb) in (((a, la), (b, lb)), (pack(pa, L), pack(pb, L))):
        want = E.distances(a, la, b, lb)
        got = dev_distance(a, la, b, lb)
        assert got.dtype == np.int32 and got.tolist() == want.tolist(), (L, R_)
        assert dev_distance(b, lb, a, la).tolist() == want.tolist(), (L, R_)  # symmetry
    want = E.distances(*pack(pa, L), *pack(pb, L)).tolist()
    assert want[:7] == [0, max(1, L // 2), max(1, L // 2), L, L, 0, 0] and want[7:9] == [1, 1]      # (the planted rows are what they claim)


def test_edit_distance_public_function_compacts_raw_rows():
    rng = np.random.default_rng(5)
    a = rng.integers(0, 64, (9, 40)) * (rng.random((9, 40)) > 0.5)
    b = np.roll(a, 3, axis=1)                                                 # the same molecules: zeros elsewhere, ids rotated
    b[0] = a[0][::-1]
    got = edit_distance(torch.from_numpy(a).short(), b.astype(np.int64), DEV)
    ca, cb = R.compact(a), R.compact(b)
    assert got.dtype == torch.int64 and got.device.type == "cuda"
    assert got.cpu().tolist() == E.distances(ca[0], ca[1], cb[0], cb[1]).tolist()


# ----------------------------------------------------------------------------------------------------------------------
# mdt::edit_nearest
# ----------------------------------------------------------------------------------------------------------------------
def dev_nearest(q, lq, k, lk):
    d, i = torch.ops.mdt.edit_nearest(dev(q), dev(lq), dev(k), dev(lk))
    assert d.dtype == i.dtype == torch.int32
    return d.cpu().numpy(), i.cpu().numpy()


@pytest.mark.parametrize("R_", [1, 5, 67])
@pytest.mark.parametrize("M_", [1, 2, CHUNK, CHUNK + 1])
def test_edit_nearest_matches_brute_force(M_, R_):
    rng = np.random.default_rng(10 * M_ + R_)
    L = 8 if M_ >= CHUNK else 64
    # the bulk: ids below 6, so equal distances are common; the planted rows use ids from 48 up, at least L - 1 edits from the bulk
    known = [rng.integers(1, 6, rng.integers(0, L + 1)).tolist() for _ in range(M_)]
    query = [rng.integers(1, 6, rng.integers(0, L + 1)).tolist() for _ in range(R_)]
    member = [63] + rng.integers(48, 63, L - 1).tolist()                      # a query that is in the set, once
    at = M_ - 2 if M_ >= CHUNK else M_ - 1
    known[at] = member
    query[0] = member
    if M_ >= CHUNK:
        # q1: two known rows one substitution away, the first in the first wave's share, the second the LAST row -- with
        # M = CHUNK + 1 the one row of the second chunk: equal distances on both sides of the boundary, the lower index wins.
        # q2: two edits from the first of them and one from the last: the later chunk wins on distance.
        q1 = list(range(56, 64))
        x5, xl = [55] + q1[1:], q1[:-1] + [55]
        q2 = [54] + xl[1:]
        known[5], known[M_ - 1] = x5, xl
        for r, q in ((1, q1), (2, q2)):
            if r < R_:
                query[r] = q
    (q, lq), (k, lk) = pack(query, L), pack(known, L)
    want_d, want_i = E.nearest(q, lq, k, lk)
    got_d, got_i = dev_nearest(q, lq, k, lk)
    assert got_d.tolist() == want_d.tolist() and got_i.tolist() == want_i.tolist()
    assert (got_d[0], got_i[0]) == (0, at)
    if M_ >= CHUNK and R_ > 2:
        assert (got_d[1], got_i[1]) == (1, 5) and (got_d[2], got_i[2]) == (1, M_ - 1)
    again = dev_nearest(q, lq, k, lk)
    assert np.array_equal(again[0], got_d) and np.array_equal(again[1], got_i)


def test_nearest_known_on_raw_rows():
    rng = np.random.default_rng(9)
    L = 12
    raw_known = rng.integers(1, 5, (40, L + 3)) * (rng.random((40, L + 3)) > 0.45)       # interior zeros; some rows too long for L
    raw = rng.integers(1, 5, (9, L)) * (rng.random((9, L)) > 0.4)
    raw[0] = 0                                                                # the empty molecule: as far as the shortest known one
    ks = KnownSet(raw_known, L)
    raw[1, :] = 0
    raw[1, L - ks.lengths[3]:] = ks.packed[3, :ks.lengths[3]]                 # a member, its zeros in front
    d, i = nearest_known(raw, ks, DEV)
    q, lq, _, _ = R.compact(raw)
    want_d, want_i = E.nearest(q, lq, ks.packed, ks.lengths)
    assert d.dtype == i.dtype == torch.int64 and d.cpu().tolist() == want_d.tolist() and i.cpu().tolist() == want_i.tolist()
    assert int(d[0]) == int(ks.lengths.min()) and (int(d[1]), int(i[1])) == (0, 3)
    d2, i2 = nearest_known(torch.from_numpy(raw).to(DEV), raw_known, DEV)     # raw ids are wrapped into the same set
    assert torch.equal(d2, d) and torch.equal(i2, i)


# ----------------------------------------------------------------------------------------------------------------------
# mdt::screen_select_diverse
# ----------------------------------------------------------------------------------------------------------------------
def dev_diverse(score, ids, N, K, known=None, known_dist=None, min_novelty=1, min_distance=1):
    packed, length, key, _ = torch.ops.mdt.tokens_compact(dev(ids, torch.int64), 0, 1.0)
    kk = known.on(DEV) if known is not None and len(known) else (None, None, None)
    kd = None if known_dist is None else dev(known_dist)
    out = torch.ops.mdt.screen_select_diverse(dev(score, torch.float32), key, packed, length, N, K, *kk, kd, min_novelty, min_distance)
    plain = torch.ops.mdt.screen_select(dev(score, torch.float32), key, packed, length, N, K, *kk)
    return tuple(t.cpu().numpy() for t in out), tuple(t.cpu().numpy() for t in plain)


def ref_diverse(score, ids, N, K, known_rows=(), known_dist=None, min_novelty=1, min_distance=1):
    packed, length, _, _ = R.compact(ids)
    known = [tuple(int(t) for t in r if t) for r in known_rows]
    return E.select_diverse(score, packed, length, N, ids.shape[0] // N, K, known, known_dist, min_novelty, min_distance)


def agree(got, want, what=None):
    for a, b, name in zip(got, want, ("status", "index", "count")):
        assert a.dtype == b.dtype and np.array_equal(a, b), (name, what)


def select_inputs(rng, N, G, L=12):
    """Candidates as the generator of the select tests makes them: molecules from a pool (pairs and triples occur), the empty
    one among them, some with their zeros elsewhere; scores with exact ties, a NaN and an infinity."""
    pool = rng.integers(1, 16, (max(2, N // 2), L)) * (rng.random((max(2, N // 2), L)) > 0.3)
    pool[0] = 0
    ids = pool[rng.integers(len(pool), size=N * G)]
    shift = rng.random(N * G) < 0.3
    ids[shift] = np.roll(ids[shift], 3, axis=1)
    score = rng.choice(np.array([0.25, 0.5, 0.5, 1.0, 2.0, 3.5, np.nan, np.inf], np.float32), N * G)
    return ids, score


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("N", [1, 5, 70])
def test_diverse_select_at_distance_one_is_the_plain_select(N, G):
    rng = np.random.default_rng(10 * N + G)
    for M_ in (0, 7):
        ids, score = select_inputs(rng, N, G)
        known_rows = rng.integers(1, 16, (M_, 14)) * (rng.random((M_, 14)) > 0.4) if M_ else np.zeros((0, 12), np.int64)
        ks = KnownSet(known_rows, 12)
        if M_:
            ids[N * G // 2] = ks.packed[len(ks) // 2]
        for K in sorted({1, min(2, N), N}):
            for d in (1, 0):
                got, plain = dev_diverse(score, ids, N, K, ks, min_distance=d)
                agree(got, plain, (M_, K, d))
                agree(got, ref_diverse(score, ids, N, K, ks.packed), (M_, K, d))
            if M_:
                assert (got[0] & R.KNOWN).any()


def crafted_groups():
    """G = 2, N = 8, L = 8, row c * 2 + g.  Group 0: A, A' (one substitution), B (far), A'' (2 from A, 1 from A'), C tying with B,
    a NaN one substitution from A, an empty row, a repeat of A'.  Group 1: eight rows one substitution apart."""
    A, A1, B, A2, C = [1, 2, 3, 4, 5], [1, 2, 3, 4, 6], [7] * 6, [1, 2, 3, 9, 6], [8, 8, 8]
    g0 = [A, A1, B, A2, C, [1, 2, 3, 4, 7], [], A1]
    s0 = [0.1, 0.2, 0.3, 0.4, 0.3, np.nan, 0.0, 0.0]
    g1 = [[1, 2, t] for t in range(3, 11)]
    s1 = [0.8, 0.7, 0.6, 0.5, 0.4, 0.3, 0.2, 0.2]                             # best: c = 6 (the tie with c = 7 goes to the lower c)
    ids = np.zeros((16, 8), np.int64)
    score = np.zeros(16, np.float32)
    for c in range(8):
        for g, (rows, sc) in enumerate(((g0, s0), (g1, s1))):
            ids[c * 2 + g, 8 - len(rows[c]):] = rows[c]                       # (zeros in front: compaction is part of the path)
            score[c * 2 + g] = sc[c]
    return ids, score


def test_diverse_select_on_crafted_groups():
    ids, score = crafted_groups()
    N, K, L = 8, 4, 8
    for d in (2, 3, L + 1):
        got, _ = dev_diverse(score, ids, N, K, min_distance=d)
        agree(got, ref_diverse(score, ids, N, K, min_distance=d), d)
        st = got[0].reshape(N, 2)
        assert st[5:, 0].tolist() == [R.NONFINITE, R.EMPTY, R.DUPLICATE]      # never bit 16 on what is not eligible
        assert got[1][1].tolist() == [6, -1, -1, -1] and got[2][1] == 1       # group 1 cannot fill K; the tie went to the lower c
        assert st[:, 1].tolist() == [E.CLOSE] * 6 + [0, E.CLOSE]
        if d == 2:                                                            # A' skipped; A'' is close to A' only: kept; B before C
            assert st[:5, 0].tolist() == [0, E.CLOSE, 0, 0, 0] and got[1][0].tolist() == [0, 2, 4, 3] and got[2][0] == 4
        if d == 3:
            assert st[:5, 0].tolist() == [0, E.CLOSE, 0, E.CLOSE, 0] and got[1][0].tolist() == [0, 2, 4, -1] and got[2][0] == 3
        if d == L + 1:                                                        # no two rows of width L lie further apart than L
            assert got[2].tolist() == [1, 1] and got[1][0].tolist() == [0, -1, -1, -1]
    # K = 1: the bits do not depend on where the slots ran out
    got, _ = dev_diverse(score, ids, N, 1, min_distance=2)
    agree(got, ref_diverse(score, ids, N, 1, min_distance=2))
    assert got[0].reshape(N, 2)[:5, 0].tolist() == [0, E.CLOSE, 0, 0, 0] and got[1].tolist() == [[0], [6]]


@pytest.mark.parametrize("N,G,L,top", [(5, 3, 6, 4), (70, 3, 6, 4), (12, 1, 64, 3), (600, 1, 12, 16)])
def test_diverse_select_matches_the_reference(N, G, L, top):
    """ids below ``top``: a small alphabet makes near neighbours common; L = 64: full-width rows; (600, 16): more than 256 kept
    rows, the stride of the threads over the kept list."""
    rng = np.random.default_rng(N + G + L)
    ids = rng.integers(1, top, (N * G, L)) * (rng.random((N * G, L)) > 0.25)
    ids[rng.integers(N * G)] = 0
    if N == 600:
        score, Ks, ds = rng.random(N * G).astype(np.float32), (N,), (2,)
    else:
        score = rng.choice(np.array([0.25, 0.5, 0.5, 1.0, 2.0, 3.5, np.nan], np.float32), N * G)
        Ks, ds = (N,) if L == 64 else sorted({1, 2, N}), (2, 3, L + 1)
    for K in Ks:
        for d in ds:
            got, _ = dev_diverse(score, ids, N, K, min_distance=d)
            agree(got, ref_diverse(score, ids, N, K, min_distance=d), (K, d))
            if d == L + 1:
                assert (got[2] <= 1).all()
    if N == 600:
        assert got[2][0] > 256


@pytest.mark.parametrize("min_novelty", [1, 2, 4])
def test_diverse_select_known_distance_and_known_set(min_novelty):
    rng = np.random.default_rng(min_novelty)
    N, G, K = 70, 3, 5
    ids, score = select_inputs(rng, N, G)
    ks = KnownSet(rng.integers(1, 16, (7, 12)) * (rng.random((7, 12)) > 0.4), 12)
    ids[4], ids[N * G - 2] = ks.packed[0], ks.packed[len(ks) - 1]
    known_dist = rng.integers(0, 6, N * G).astype(np.int32)
    for known in (None, ks):
        for d in (1, 3):
            got, plain = dev_diverse(score, ids, N, K, known, known_dist, min_novelty, d)
            want = ref_diverse(score, ids, N, K, () if known is None else ks.packed, known_dist, min_novelty, d)
            agree(got, want, (known is not None, d))
            near = known_dist < min_novelty
            assert (((got[0] & R.KNOWN) != 0) == (near | ((plain[0] & R.KNOWN) != 0))).all()


# ----------------------------------------------------------------------------------------------------------------------
# end to end
# ----------------------------------------------------------------------------------------------------------------------
N_, G_, K_, T_ = 5, 3, 3, 4


@pytest.fixture(scope="module")
def chain():
    inv, fwd = make_model("cfg1"), make_model("cfg3")
    inv.kernel_choice = fwd.kernel_choice = "narrow"
    cond = synth_normal("screen/cond", (G_, 12))
    tokens = inv.sample_tokens(cond.repeat(N_, 1), DEV, cond_scale=1.0, timesteps=T_, noise=NoiseSource(seed=11, sample0=7))
    return inv, fwd, cond, tokens


def by_hand(fwd, tokens, cond, known=(), **filters):
    """ids -> predict_properties_from_tokens -> to the host -> the numpy reference."""
    props = predict_properties_from_tokens(fwd, tokens, DEV, timesteps=T_, X_norm_factor=16.0, context_embedding_max_length=cond.shape[1],
                                           noise=NoiseSource(seed=12))
    return E.screen(tokens.cpu().numpy(), props.cpu().numpy(), cond.numpy(), tokens.shape[0] // cond.shape[0], K_, None, known, **filters)


def assert_screened(out, want):
    assert out.tokens.dtype == out.index.dtype == out.count.dtype == torch.int64 and out.status.dtype == torch.uint8
    for name in ("tokens", "index", "count", "status"):
        assert np.array_equal(getattr(out, name).cpu().numpy(), want[name]), name
    for name in ("props", "score"):
        got = getattr(out, name).cpu().numpy()
        assert got.shape == want[name].shape and np.array_equal(got.view(np.uint32), want[name].view(np.uint32)), name


def one_id_changed(rows, at):
    """Copies of ``rows`` with the non-zero id at place ``at`` (counted from the back) replaced by another id in [1, 16)."""
    rows = rows.clone()
    for row in rows:
        p = int(row.nonzero()[-1 - at])
        row[p] = row[p] % 15 + 1
    return rows


KW = dict(forward_timesteps=T_, X_norm_factor=16.0, forward_noise=NoiseSource(seed=12))


def test_screen_candidates_with_both_filters_equals_the_chain_by_hand(chain):
    inv, fwd, cond, tokens = chain
    assert int((tokens != 0).sum(dim=1).min()) >= 3
    # the known set: the run's own first candidate block with one id changed -- one edit from a candidate, equal to none
    known = one_id_changed(tokens[:G_], 0).cpu()
    ks = KnownSet(known, 64)
    out = screen_candidates(inv, fwd, cond, DEV, N_, K_, timesteps=T_, noise=NoiseSource(seed=11, sample0=7), known_tokens=ks,
                            min_distance=3, min_novelty=2, **KW)
    assert_screened(out, by_hand(fwd, tokens, cond, known=known.numpy(), min_distance=3, min_novelty=2))
    exact = screen_candidates(inv, fwd, cond, DEV, N_, K_, timesteps=T_, noise=NoiseSource(seed=11, sample0=7), known_tokens=ks, **KW)
    newly = ((out.status & R.KNOWN) != 0) & ((exact.status & R.KNOWN) == 0)
    assert bool(newly[0].all())                                               # the novelty filter bites where the exact lookup does not
    assert float(((out.status & 8) == 0).float().mean()) < float(((exact.status & 8) == 0).float().mean())
    # (1, 1) is today's call, bit for bit
    same = screen_candidates(inv, fwd, cond, DEV, N_, K_, timesteps=T_, noise=NoiseSource(seed=11, sample0=7), known_tokens=ks,
                             min_distance=1, min_novelty=1, **KW)
    for a, b in zip(same, exact):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_screen_tokens_diverse_on_near_copies_equals_the_chain_by_hand(chain):
    """Candidate blocks 1 and 2 are block 0 with one and with two ids changed, so within every group three candidates lie within
    two edits of each other: min_distance = 3 passes over two of them; the known set is block 3 with one id changed."""
    _, fwd, cond, tokens = chain
    tokens = tokens.clone()
    tokens[G_:2 * G_] = one_id_changed(tokens[:G_], 0)
    tokens[2 * G_:3 * G_] = one_id_changed(tokens[G_:2 * G_], 1)
    known = one_id_changed(tokens[3 * G_:4 * G_], 0).cpu()
    out = screen_tokens_diverse(fwd, tokens, cond, DEV, N_, K_, known_tokens=known, min_distance=3, min_novelty=2, **KW)
    want = by_hand(fwd, tokens, cond, known=known.numpy(), min_distance=3, min_novelty=2)
    assert (want["status"] & E.CLOSE).any() and (want["status"][3] & R.KNOWN).all()      # both filters bite
    assert_screened(out, want)
    assert int(((out.status & rt.SCREEN_CLOSE) != 0).sum()) >= G_
    only = screen_tokens_diverse(fwd, tokens, cond, DEV, N_, K_, known_tokens=known, min_distance=3, **KW)
    assert_screened(only, by_hand(fwd, tokens, cond, known=known.numpy(), min_distance=3))
    assert not bool((only.status & R.KNOWN).any())                            # ... which the exact lookup alone does not see
