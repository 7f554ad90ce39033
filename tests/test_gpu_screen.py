"""-m gpu: the screening kernels (csrc/k_screen.hip) and screen_tokens() / screen_candidates() on the device.  Every comparison
is exact, against the numpy reference tests/screen_ref.py; the end-to-end runs are compared with sample_tokens ->
predict_properties_from_tokens -> that reference on the host, bit for bit under a pinned kernel_choice."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from gpu_util import DEV, make_model
import screen_ref as R
from moleculediffusiontransformer_amd import (KnownSet, NoiseSource, predict_properties_from_tokens, screen_candidates,
                                              screen_tokens, tokens_to_forward_input)
from moleculediffusiontransformer_amd import ops  # noqa: F401  (registers torch.ops.mdt.*)
from moleculediffusiontransformer_amd.synth import synth_normal

pytestmark = pytest.mark.gpu


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def rows_for(rng, B, L):
    """Random ids in [0, 16) with about 40 % zeros; the first rows are all zero, all non-zero and alternating."""
    ids = rng.integers(1, 16, (B, L)) * (rng.random((B, L)) > 0.4)
    special = [np.zeros(L, np.int64), rng.integers(1, 16, L), np.arange(L) % 2 * rng.integers(1, 16, L)]
    for b, row in enumerate(special[:B]):
        ids[b] = row
    return ids, special


def check_compact(ids, Lf, x_norm):
    packed, length, key, fwd = torch.ops.mdt.tokens_compact(torch.from_numpy(ids).to(DEV), Lf, x_norm)
    rp, rl, rk, rf = R.compact(ids, Lf, x_norm)
    what = (ids.shape, Lf, x_norm)
    assert packed.dtype == torch.int32 and np.array_equal(packed.cpu().numpy(), rp), what
    assert length.dtype == torch.int32 and np.array_equal(length.cpu().numpy(), rl), what
    assert np.array_equal(u64(key), rk), what                                # device keys == host keys
    assert fwd.shape == (ids.shape[0], Lf) and np.array_equal(fwd.cpu().numpy().view(np.uint32), rf.view(np.uint32)), what


# ----------------------------------------------------------------------------------------------------------------------
# mdt_tokens_compact
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 5])                    # 5: no multiple of the four rows of a block
@pytest.mark.parametrize("L", [1, 63, 64, 65, 130])      # the 64-lane chunk boundary and the carry across chunks
def test_compact_matches_the_reference(L, B):
    rng = np.random.default_rng(100 * L + B)
    ids, special = rows_for(rng, B, L)
    batches = [ids] if B > 1 else [ids] + [row[None] for row in special]      # B = 1: every special row on its own
    for batch in batches:
        for Lf in sorted({0, max(1, L // 2), L, L + 7}):                     # no forward input; Lf below, equal to, above L
            for x_norm in ((1.0, 16.0, 3.0) if Lf else (1.0,)):              # 3: an inexact divide, rounded double -> float
                check_compact(batch, Lf, x_norm)


def test_compact_forward_input_is_tokens_to_forward_input():
    g = load_golden("token_chain.npz")
    ids, L, xn = torch.from_numpy(g["ids"]).to(DEV), int(g["max_length"]), float(g["X_norm_factor"])
    for Lf in (L, L - 9, L + 5):
        for x_norm in (xn, 1.0, 3.0):
            fwd = torch.ops.mdt.tokens_compact(ids, Lf, x_norm)[3]
            assert torch.equal(fwd.view(torch.int32), tokens_to_forward_input(ids, Lf, x_norm).view(torch.int32)), (Lf, x_norm)
    assert torch.equal(torch.ops.mdt.tokens_compact(ids.int(), L, xn)[3].cpu(), torch.from_numpy(g["forward_input"]))
    # host keys of the package (KnownSet) == device keys
    ks = KnownSet(g["ids"], L)
    packed, length, key, _ = torch.ops.mdt.tokens_compact(ids, 0, 1.0)
    dev = {tuple(packed[b, :length[b]].tolist()): int(u64(key)[b]) for b in range(ids.shape[0])}
    assert {tuple(ks.packed[i, :ks.lengths[i]].tolist()): int(ks.key[i]) for i in range(len(ks))} == dev


# ----------------------------------------------------------------------------------------------------------------------
# mdt_screen_score
# ----------------------------------------------------------------------------------------------------------------------
def same_floats(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.isnan(a), np.isnan(b))


@pytest.mark.parametrize("N", [1, 5])
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("n", [1, 12, 13])
def test_score_matches_the_reference(n, G, N):
    rng = np.random.default_rng(1000 * n + 10 * G + N)
    stride = n + 5                                                           # row_stride > n: the forward sample read in place
    target = rng.standard_normal((G, n)).astype(np.float32)
    weights = rng.random(n).astype(np.float32)
    weights[0] = 0.0
    for plant in (None, np.nan, np.inf, -np.inf):
        props = rng.standard_normal((N * G, stride)).astype(np.float32)
        if plant is not None:
            props[rng.integers(N * G), rng.integers(n)] = plant
        for w in (None, weights):
            for shape in ((N * G, stride), (N * G, 1, stride)):              # (B, Lf) and the sample's own (B, 1, Lf)
                got = torch.ops.mdt.screen_score(torch.from_numpy(props).to(DEV).view(shape), torch.from_numpy(target).to(DEV),
                                                 None if w is None else torch.from_numpy(w).to(DEV), N)
                assert got.dtype == torch.float32 and same_floats(got.cpu().numpy(), R.score(props, target, w, N)), (plant, w is None)


# ----------------------------------------------------------------------------------------------------------------------
# mdt_screen_select
# ----------------------------------------------------------------------------------------------------------------------
def dev_select(score, ids, N, K, known=None, key=None):
    """status, index, count of the device for candidates ``ids`` (N * G, L) with ``score``; ``known``: a KnownSet or the three
    device tensors; ``key``: forged keys instead of the rows' own."""
    packed, length, own, _ = torch.ops.mdt.tokens_compact(torch.from_numpy(ids).to(DEV), 0, 1.0)
    kk = (None, None, None) if known is None else known.on(DEV) if isinstance(known, KnownSet) else known
    if isinstance(known, KnownSet) and len(known) == 0:
        kk = (None, None, None)
    st, idx, cnt = torch.ops.mdt.screen_select(torch.from_numpy(score).to(DEV), own if key is None else key, packed, length, N, K, *kk)
    torch.cuda.synchronize()
    return st.cpu().numpy(), idx.cpu().numpy(), cnt.cpu().numpy()


def ref_select(score, ids, N, K, known_rows=()):
    packed, length, _, _ = R.compact(ids)
    G = ids.shape[0] // N
    return R.select(score, packed, length, N, G, K, [tuple(int(t) for t in r if t) for r in known_rows])


def agree(got, want, what=None):
    for a, b, name in zip(got, want, ("status", "index", "count")):
        assert a.dtype == b.dtype and np.array_equal(a, b), (name, what)


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("N", [1, 2, 255, 256, 257, 1024])                   # around the stride of the 256 threads; the limit
def test_select_matches_the_reference(N, G):
    rng = np.random.default_rng(10 * N + G)
    L = 12
    pool = rng.integers(1, 16, (max(2, N // 2), L)) * (rng.random((max(2, N // 2), L)) > 0.3)     # molecules: pairs, triples occur
    pool[0] = 0                                                               # the empty molecule
    for M in (0, 1, 7):
        ids = pool[rng.integers(len(pool), size=N * G)]
        shift = rng.random(N * G) < 0.3                                       # the same molecule with its zeros elsewhere
        ids[shift] = np.roll(ids[shift], 3, axis=1)
        score = rng.choice(np.array([0.25, 0.5, 0.5, 1.0, 2.0, 3.5, np.nan, np.inf], np.float32), N * G)      # exact ties
        known_rows = rng.integers(1, 16, (M, L + 2)) * (rng.random((M, L + 2)) > 0.4) if M else np.zeros((0, L), np.int64)
        ks = KnownSet(known_rows, L)
        if M == 7:
            assert len(ks) >= 3
            # known molecules among the candidates: the FIRST and the LAST entry of the sorted array, and one from inside
            for at, entry in ((0, 0), (N * G - 1, len(ks) - 1), (N * G // 2, len(ks) // 2)):
                ids[at] = np.roll(ks.packed[entry][:L], 1) if ks.lengths[entry] < L else ks.packed[entry]
        elif M == 1 and N * G > 1 and len(ks):
            ids[1] = ks.packed[0]
        for K in sorted({1, N}):
            got = dev_select(score, ids, N, K, ks)
            agree(got, ref_select(score, ids, N, K, ks.packed), (M, K))
            if M == 7 and N * G >= 3:
                assert all(got[0][at] & R.KNOWN for at in (0, N * G - 1, N * G // 2))
            assert got[1].shape == (G, K) and ((got[1] >= 0).sum(axis=1) == got[2]).all()


def test_select_ties_duplicates_and_short_groups():
    # G = 3, N = 6, row c * 3 + g.  group 0: nothing eligible; group 1: two eligible, fewer than K; group 2: ties and a triple
    A, B_, C, D, E, Z = [1, 2, 3, 0], [1, 2, 0, 3], [3, 2, 1, 0], [0, 0, 0, 7], [7, 0, 0, 0], [0, 0, 0, 0]
    mol = {0: [Z, A, A, A, B_, Z],                # empty | non-finite | duplicates of a NON-eligible first occurrence | empty
           1: [A, C, B_, D, E, Z],                # A (eligible), C (eligible), B_ == A, D non-finite, E == D (dup of a non-finite), empty
           2: [D, A, E, C, B_, D]}                # D, A, E == D, C, B_ == A, D again: a triple of D
    sc = {0: [1.0, np.nan, 0.5, 0.25, 0.1, 0.0],
          1: [2.0, 1.0, 0.5, np.inf, 0.1, 0.0],
          2: [0.5, 0.5, 0.1, 0.5, 0.0, 0.0]}      # D, A, C tie at 0.5: the lower c first
    N, G, K = 6, 3, 4
    ids = np.array([mol[g][c] for c in range(N) for g in range(G)], np.int64)
    score = np.array([sc[g][c] for c in range(N) for g in range(G)], np.float32)
    status, index, count = dev_select(score, ids, N, K)
    agree((status, index, count), ref_select(score, ids, N, K))
    st = status.reshape(N, G)
    assert st[:, 0].tolist() == [1, 2, 4, 4, 4, 5] and st[:, 1].tolist() == [0, 0, 4, 2, 4, 1] and st[:, 2].tolist() == [0, 0, 4, 0, 4, 4]
    assert index.tolist() == [[-1, -1, -1, -1], [1, 0, -1, -1], [0, 1, 3, -1]] and count.tolist() == [0, 2, 3]


def test_select_never_trusts_the_key():
    """Forced key collisions: every candidate carries the SAME key, so only the comparison of length and packed row can tell
    molecules apart -- nothing but the true repeats may be flagged; and a run of three equal known keys whose LAST entry is the
    match (with smaller and larger keys around the run) must be scanned to its end."""
    rng = np.random.default_rng(7)
    N, G, L = 9, 2, 10
    ids = rng.integers(1, 16, (N * G, L)) * (rng.random((N * G, L)) > 0.3)
    ids[6], ids[8] = ids[2], ids[0] * (np.arange(L) != np.flatnonzero(ids[0])[-1])      # a true repeat in group 0; a prefix of row 0
    ids[5] = ids[1] * (np.arange(L) != np.flatnonzero(ids[1])[0])             # one id fewer than row 1: a different molecule
    score = rng.random(N * G).astype(np.float32)
    forged = torch.full((N * G,), 0x1234_5678_9ABC, dtype=torch.int64, device=DEV)
    got = dev_select(score, ids, N, 3, key=forged)
    agree(got, ref_select(score, ids, N, 3))
    assert got[0].tolist() == [4 if r == 6 else 0 for r in range(N * G)]
    # the known run: keys [k - 5, k, k, k, k + 5]; entries 1 and 2 are other molecules (one of the same length), entry 3 is row 4;
    # then a run that ends before entry 3 (its entry 0 is row 3), and a run of entry 3 alone
    packed, length, _, _ = R.compact(ids)
    other = packed[4].copy()
    other[0] = other[0] % 15 + 1                                              # same length, one id differs
    known_rows = np.stack([packed[3], other, packed[7][::-1] * 0 + 9, packed[4], packed[11]])
    kp, kl, _, _ = R.compact(known_rows)
    k = 0x1234_5678_9ABC
    for keys, want_known in (([k - 5, k, k, k, k + 5], {4}), ([k, k, k, k + 1, k + 5], {3}), ([k - 9, k - 5, k - 1, k, k + 5], {4})):
        known = (torch.tensor(keys, dtype=torch.int64, device=DEV), torch.from_numpy(kp).to(DEV), torch.from_numpy(kl).to(DEV))
        status = dev_select(score, ids, N, 3, known=known, key=forged)[0]
        assert {r for r in range(N * G) if status[r] & R.KNOWN} == want_known, keys
        assert [s & ~R.KNOWN for s in status.tolist()] == got[0].tolist()
    # keys with the top bit set sort as UNSIGNED numbers: a known key 2^63 + 1 lies above key 5
    top = -(1 << 63) + 1
    known = (torch.tensor([5, top], dtype=torch.int64, device=DEV), torch.from_numpy(kp[[0, 3]].copy()).to(DEV),
             torch.from_numpy(kl[[0, 3]].copy()).to(DEV))
    status = dev_select(score, ids, N, 3, known=known, key=torch.full((N * G,), top, dtype=torch.int64, device=DEV))[0]
    assert {r for r in range(N * G) if status[r] & R.KNOWN} == {4}


# ----------------------------------------------------------------------------------------------------------------------
# end to end
# ----------------------------------------------------------------------------------------------------------------------
N_, G_, K_, T_ = 5, 3, 2, 4


@pytest.fixture(scope="module")
def chain():
    inv, fwd = make_model("cfg1"), make_model("cfg3")
    inv.kernel_choice = fwd.kernel_choice = "narrow"
    return inv, fwd, synth_normal("screen/cond", (G_, 12))


def by_hand(fwd, tokens, cond, known=(), weights=None, keep=K_):
    """The parent's way: ids -> predict_properties_from_tokens -> to the host -> the numpy reference."""
    props = predict_properties_from_tokens(fwd, tokens, DEV, timesteps=T_, X_norm_factor=16.0, context_embedding_max_length=cond.shape[1],
                                           noise=NoiseSource(seed=12))
    return R.screen(tokens.cpu().numpy(), props.cpu().numpy(), cond.numpy(), tokens.shape[0] // cond.shape[0], keep, weights, known)


def assert_screened(out, want):
    assert out.tokens.dtype == out.index.dtype == out.count.dtype == torch.int64 and out.status.dtype == torch.uint8
    assert out.props.dtype == out.score.dtype == torch.float32
    for name in ("tokens", "index", "count", "status"):
        assert np.array_equal(getattr(out, name).cpu().numpy(), want[name]), name
    for name in ("props", "score"):
        got = getattr(out, name).cpu().numpy()
        assert got.shape == want[name].shape and np.array_equal(got.view(np.uint32), want[name].view(np.uint32)), name


def test_screen_candidates_equals_the_chain_by_hand(chain):
    inv, fwd, cond = chain
    kw = dict(timesteps=T_, forward_timesteps=T_, X_norm_factor=16.0, forward_noise=NoiseSource(seed=12))
    out = screen_candidates(inv, fwd, cond, DEV, N_, K_, noise=NoiseSource(seed=11, sample0=7), **kw)
    tokens = inv.sample_tokens(cond.repeat(N_, 1), DEV, cond_scale=1.0, timesteps=T_, noise=NoiseSource(seed=11, sample0=7))
    assert_screened(out, by_hand(fwd, tokens, cond))
    assert out.tokens.shape == (G_, K_, 64) and out.props.shape == (G_, K_, 12) and out.status.shape == (N_, G_)
    assert int(out.count.min()) >= 1                                           # (there is something to choose from)
    # weights reach the score
    w = [0.0] * 11 + [2.0]
    assert_screened(screen_candidates(inv, fwd, cond, DEV, N_, K_, noise=NoiseSource(seed=11, sample0=7), weights=w, **kw),
                    by_hand(fwd, tokens, cond, weights=np.array(w, np.float32)))
    # a known set of two of the returned molecules: flagged, and never returned
    known = torch.stack([out.tokens[0, 0], out.tokens[G_ - 1, 0]]).cpu()
    again = screen_candidates(inv, fwd, cond, DEV, N_, K_, noise=NoiseSource(seed=11, sample0=7), known_tokens=KnownSet(known, 64), **kw)
    assert_screened(again, by_hand(fwd, tokens, cond, known=known.numpy()))
    mols = {tuple(t for t in row.tolist() if t) for row in known}
    flagged = (again.status.cpu() & R.KNOWN) != 0
    assert bool(flagged[int(out.index[0, 0]), 0]) and bool(flagged[int(out.index[G_ - 1, 0]), G_ - 1])
    for g in range(G_):
        for k in range(int(again.count[g])):
            assert tuple(t for t in again.tokens[g, k].tolist() if t) not in mols
    assert float(((again.status & 8) == 0).float().mean()) < 1.0              # the reference's fraction of novel structures


def test_one_guidance_scale_per_candidate_block(chain):
    inv, fwd, cond = chain
    scales = [2.0, 1.0, 7.5, 2.0, 1.0]
    # the scalar calls first: block c is the call at scales[c] whose sample0 is sample0 + c * G
    blocks = [inv.sample_tokens(cond, DEV, cond_scale=s, timesteps=T_, noise=NoiseSource(seed=11, sample0=7 + c * G_))
              for c, s in enumerate(scales)]
    out = screen_candidates(inv, fwd, cond, DEV, N_, K_, cond_scale=scales, timesteps=T_, noise=NoiseSource(seed=11, sample0=7),
                            forward_timesteps=T_, X_norm_factor=16.0, forward_noise=NoiseSource(seed=12))
    assert_screened(out, by_hand(fwd, torch.cat(blocks), cond))


def test_fixture_novelty_through_screen_tokens(chain):
    """tests/golden/screen.npz: the status bits of screen_tokens against the reference's own is_novel and string equality."""
    _, fwd, _ = chain
    g = load_golden("screen.npz")
    ids, cond = torch.from_numpy(g["ids"]), synth_normal("screen/cond", (1, 12))
    out = screen_tokens(fwd, ids, cond, DEV, 40, 40, known_tokens=g["known_ids"], forward_timesteps=T_, X_norm_factor=16.0,
                        forward_noise=NoiseSource(seed=12))
    status = out.status.cpu().numpy()[:, 0]
    assert ((status & R.KNOWN) == 0).tolist() == g["novel"].tolist()
    assert ((status & R.DUPLICATE) != 0).tolist() == (g["first"] != np.arange(40)).tolist()
    assert ((status & R.EMPTY) != 0).tolist() == [s == "" for s in g["smiles"]]
    assert_screened(out, by_hand(fwd, ids.to(DEV), cond, known=g["known_ids"], keep=40))
