"""-m gpu: mdt_smiles_check (csrc/k_smiles.hip), the `reject` input of the two selections (csrc/k_screen.hip) and the screening
calls with ``vocabulary=`` on the device.  Every comparison is exact: status and position against the string-level reference
tests/smiles_ref.py, the selections against tests/screen_ref.py / tests/edit_ref.py with the reject bits OR-ed into the status."""
import numpy as np
import pytest
import torch

import edit_ref as E
import screen_ref as R
import smiles_ref as S
from gpu_util import DEV, make_model
from moleculediffusiontransformer_amd import (NoiseSource, SmilesVocabulary, screen_tokens, screen_tokens_diverse, smiles_check)
from moleculediffusiontransformer_amd import ops  # noqa: F401  (registers torch.ops.mdt.*)
from moleculediffusiontransformer_amd.synth import synth_normal

pytestmark = pytest.mark.gpu

V = SmilesVocabulary([None] + S.CHARS)


def verdicts(strings, **kw):
    """The reference on every string: (status int64 (R,), position int64 (R,)) -- each distinct string is judged once."""
    seen = {}
    out = [seen[s] if s in seen else seen.setdefault(s, S.check(s, **kw)) for s in strings]
    return np.array([o[0] for o in out], np.int64), np.array([o[1] for o in out], np.int64)


def device_verdicts(ids, vocabulary=V):
    status, position = smiles_check(ids, vocabulary, DEV)
    torch.cuda.synchronize()
    assert status.dtype == position.dtype == torch.int64 and status.shape == position.shape == (ids.shape[0],)
    return status.cpu().numpy(), position.cpu().numpy()


def agree(ids, strings, what=None, **kw):
    got, want = device_verdicts(ids), verdicts(strings, **kw)
    wrong = [(s, (int(a), int(b)), (int(c), int(d))) for s, a, b, c, d in zip(strings, got[0], got[1], want[0], want[1])
             if (a, b) != (c, d)]
    assert not wrong, (what, len(wrong), wrong[:5])                          # (string, device, reference)


@pytest.fixture(scope="module")
def mutated():
    rows = S.mutated_rows()
    return rows, verdicts(rows)


def test_the_three_tables():
    strings = [s for s, _, _ in S.TABLES]
    status, position = device_verdicts(V.encode(strings, 32))
    for (s, st, pos), a, b in zip(S.TABLES, status, position):
        assert (int(a), int(b)) == (st, pos) == S.check(s), s


def test_mutated_rows(mutated):
    rows, (status, position) = mutated
    for v in (S.OK, S.MALFORMED, S.OVERVALENT):                              # a kernel that always answers one thing cannot pass
        assert int((status == v).sum()) >= 0.05 * len(rows), v
    ids = V.encode(rows, 32)
    got = device_verdicts(ids)
    assert np.array_equal(got[0], status) and np.array_equal(got[1], position), \
        [(r, a, b, c, d) for r, a, b, c, d in zip(rows, got[0], got[1], status, position) if (a, b) != (c, d)][:5]
    again = device_verdicts(ids)                                             # two calls give equal results
    assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1])


@pytest.mark.parametrize("R_", [1, 63, 64, 65])                            # one workgroup takes 64 rows
@pytest.mark.parametrize("L", [1, 32, 33, 128])                            # the limits, and a width that is no multiple of four
def test_shapes(L, R_, mutated):
    rng = np.random.default_rng(100 * L + R_)
    pool = mutated[0]
    strings = []
    for r in range(R_):
        s = pool[int(rng.integers(len(pool)))]
        while L > 40 and len(s) < L - 30 and rng.random() < 0.8:            # wide rows: chains of several strings, up to the full width
            s = s + "." + pool[int(rng.integers(len(pool)))]
        strings.append(s[:L])
    agree(V.encode(strings, L), strings, (L, R_))


def test_long_rows_ring_numbers_and_depth():
    deep = "C(" * 42 + "C" + ")" * 42                                        # 127 tokens, depth 42
    strings = [deep + "C", deep[:-1] + "C", deep, deep[:-1], "C(" * 64, "C" * 128, "C0CC0", "C%99CC%99", "C%00CC%00", "C%63CC%64",
               "C%64CC%64", "C%99" * 32, "C1" * 64, "C" + "%12" * 42, "C$1$2$3" + "C1C2C3" * 10, "[C]" + "($C)" * 31,
               "C" + "(C)" * 42 + "C", "[13CH4]" * 18 + "CC", "C%12" + "C" * 120 + "%12", "C1" + "C" * 125 + "1"]
    assert len(strings[0]) == 128 and S.check(strings[0]) == (S.OK, -1) and S.check(strings[1]) == (S.MALFORMED, 127)
    assert S.check(deep) == (S.OK, -1) and S.check(deep[:-1]) == (S.MALFORMED, 126)
    assert S.check("C0CC0") == S.check("C%99CC%99") == (S.OK, -1)
    agree(V.encode(strings, 128), strings)


def test_zeros_between_tokens_empty_rows_and_ids_without_a_character():
    rng = np.random.default_rng(7)
    strings = [s for s, _, _ in S.TABLES]
    ids = V.encode(strings, 32).numpy()
    spread = np.zeros((len(strings), 64), np.int64)
    for r, s in enumerate(strings):                                          # the same tokens at random places, in order
        at = np.sort(rng.choice(64, len(s), replace=False))
        spread[r, at] = ids[r, :len(s)]
    for dtype in (torch.int64, torch.int32, torch.int16, torch.uint8):
        agree(torch.from_numpy(spread).to(dtype), strings, dtype)
    # length-0 rows: OK, -1 (bit 1 of the selection reports them)
    status, position = device_verdicts(torch.zeros(3, 17, dtype=torch.int64))
    assert status.tolist() == [0, 0, 0] and position.tolist() == [-1, -1, -1]
    # an id >= 256, a negative id, an id the vocabulary leaves unused: malformed where it stands in the compacted row
    C, O, op = (int(V.encode(ch, 1)[0, 0]) for ch in "CO(")
    rows = torch.tensor([[C, 256, C, 0], [C, 0, C, 300], [C, C, -5, C], [C, C, 200, 0], [0, 70000, 0, C], [C, op, 256, 0],
                         [op, 256, 0, 0], [C, O, 0, 255]], dtype=torch.int64)
    status, position = device_verdicts(rows)
    assert status.tolist() == [32] * 8 and position.tolist() == [1, 2, 2, 2, 0, 2, 0, 2]


def test_max_valence_override():
    strings = ["N(C)(C)(C)C", "C(C)(C)(C)(C)C", "N(C)(C)(C)(C)(C)C", "ClC", "Cl(C)C"]
    ids = V.encode(strings, 32)
    assert [tuple(int(x) for x in p) for p in zip(*device_verdicts(ids))] == [(64, 0), (64, 0), (64, 0), (0, -1), (64, 0)]
    five = SmilesVocabulary([None] + S.CHARS, max_valence={"N": 5, "Cl": 2})
    got = [tuple(int(x) for x in p) for p in zip(*device_verdicts(ids, five))]
    assert got == [(0, -1), (64, 0), (64, 0), (0, -1), (0, -1)]
    assert got == [S.check(s, {"N": 5, "Cl": 2}) for s in strings]


# ----------------------------------------------------------------------------------------------------------------------
# the selections with `reject`
# ----------------------------------------------------------------------------------------------------------------------
G_, N_, K_, L_ = 3, 8, 3, 32


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def ref_select_reject(score, packed, length, reject, min_distance=1):
    """screen_ref's / edit_ref's selection with the reject bits OR-ed into the status before eligibility is decided."""
    status, _, _ = R.select(score, packed, length, N_, G_, K_)
    status = status | reject
    index, count = np.full((G_, K_), -1, np.int32), np.zeros(G_, np.int32)
    for g in range(G_):
        kept = []
        for _, c in sorted((float(score[c * G_ + g]), c) for c in range(N_) if status[c * G_ + g] == 0):
            r = c * G_ + g
            rows = [o * G_ + g for o in kept]
            d = E.distances(np.tile(packed[r], (len(rows), 1)), np.full(len(rows), length[r]), packed[rows], length[rows]) if rows else []
            if min_distance > 1 and any(x < min_distance for x in d):
                status[r] |= E.CLOSE
            elif len(kept) < K_:
                kept.append(c)
        index[g, :len(kept)] = kept
        count[g] = len(kept)
    return status, index, count


@pytest.fixture(scope="module")
def candidates():
    """Synthetic scores, as tests/screen_ref.py takes them.  Group 0: candidate 2 has the best score and candidate 5 lies one edit
    from it, so at min_distance 3 candidate 2 pushes 5 out -- unless 2 is rejected.  Candidate 4 of every group is empty,
    candidate 7 repeats candidate 1."""
    rng = np.random.default_rng(3)
    ids = rng.integers(1, 20, (N_ * G_, L_)) * (np.arange(L_)[None, :] < rng.integers(6, 20, (N_ * G_, 1)))
    ids[5 * G_] = ids[2 * G_]
    ids[5 * G_, 3] = ids[2 * G_, 3] % 19 + 1
    ids[4 * G_:5 * G_] = 0
    ids[7 * G_:8 * G_] = ids[1 * G_:2 * G_]
    score = rng.random(N_ * G_).astype(np.float32)
    score[2 * G_], score[5 * G_] = 0.001, 0.002
    reject = np.zeros(N_ * G_, np.uint8)
    reject[2 * G_] = S.MALFORMED                                             # the best of group 0
    reject[1 * G_ + 1] = S.OVERVALENT                                        # candidate 1 of group 1; its repeat 7 stays a duplicate
    reject[4 * G_ + 2] = S.MALFORMED                                         # an empty row that is rejected as well: bits add up
    reject[6 * G_ + 2] = S.MALFORMED | S.OVERVALENT
    packed, length, key, _ = torch.ops.mdt.tokens_compact(dev(ids), 0, 1.0)
    return ids, score, reject, packed, length, key


def same(got, want, what):
    torch.cuda.synchronize()
    for name, g, w in zip(("status", "index", "count"), got, want):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, name, g, w)


def test_select_with_reject(candidates):
    ids, score, reject, packed, length, key = candidates
    rp, rl, _, _ = R.compact(ids)
    want = ref_select_reject(score, rp, rl, reject)
    got = torch.ops.mdt.screen_select_reject(dev(score), key, packed, length, N_, K_, None, None, None, dev(reject))
    same(got, want, "plain")
    status, index = want[0].reshape(N_, G_), want[1]
    assert status[2, 0] == 32 and 2 not in index[0] and status[1, 1] == 64 and status[7, 1] == R.DUPLICATE
    assert status[4, 2] == (R.EMPTY | 32) and status[6, 2] == 96
    # without the bits candidate 2 leads group 0
    plain = R.select(score, rp, rl, N_, G_, K_)
    assert plain[1][0, 0] == 2 and plain[1][0, 1] == 5
    # reject=None: the existing op, bit for bit
    a = torch.ops.mdt.screen_select_reject(dev(score), key, packed, length, N_, K_, None, None, None, None)
    b = torch.ops.mdt.screen_select(dev(score), key, packed, length, N_, K_, None, None, None)
    same(a, plain, "reject=None")
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    # all-zero reject bytes change nothing either
    same(torch.ops.mdt.screen_select_reject(dev(score), key, packed, length, N_, K_, None, None, None, dev(np.zeros_like(reject))),
         plain, "zero reject")


def test_diverse_select_with_reject(candidates):
    ids, score, reject, packed, length, key = candidates
    rp, rl, _, _ = R.compact(ids)
    args = (dev(score), key, packed, length, N_, K_, None, None, None, None, 1, 3)
    want = ref_select_reject(score, rp, rl, reject, min_distance=3)
    same(torch.ops.mdt.screen_select_diverse_reject(*args, dev(reject)), want, "diverse")
    # the rejected best of group 0 pushes nobody out: candidate 5, one edit from it, is kept now and was CLOSE before
    before = E.select_diverse(score, rp, rl, N_, G_, K_, min_distance=3)
    assert before[0].reshape(N_, G_)[5, 0] == E.CLOSE and before[1][0, 0] == 2 and 5 not in before[1][0]
    assert want[0].reshape(N_, G_)[2, 0] == 32 and want[0].reshape(N_, G_)[5, 0] == 0 and want[1][0, 0] == 5
    # reject=None: the existing op, bit for bit
    a = torch.ops.mdt.screen_select_diverse_reject(*args, None)
    b = torch.ops.mdt.screen_select_diverse(*args)
    same(a, before, "reject=None")
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ----------------------------------------------------------------------------------------------------------------------
# end to end
# ----------------------------------------------------------------------------------------------------------------------
def test_screening_with_a_vocabulary_end_to_end():
    """Hand-made rows whose meaning the vocabulary decides: candidate row r carries the id 20 + r, an 'N' in every row but one."""
    G2, N2, K2, L2, T = 2, 4, 2, 32, 4
    fwd = make_model("cfg3")
    fwd.kernel_choice = "narrow"
    cond = synth_normal("screen/cond", (G2, 12))
    C, O = 1, 2
    tokens = torch.zeros(N2 * G2, L2, dtype=torch.int64)
    for r in range(N2 * G2):
        tokens[r, :4 + r % 3] = torch.tensor([C, C, 20 + r, O, C, C][:4 + r % 3])
    kw = dict(forward_timesteps=T, X_norm_factor=16.0)
    noise = lambda: NoiseSource(seed=12)   # noqa: E731
    full = screen_tokens(fwd, tokens, cond, DEV, N2, N2, forward_noise=noise(), **kw)          # the whole order of every target
    assert full.count.tolist() == [N2] * G2
    best = int(full.index[0, 0])                                                                # the best candidate of target 0 ...
    chars = {C: "C", O: "O", **{20 + r: "N" for r in range(N2 * G2)}}
    chars[20 + best * G2] = "("                                                                 # ... reads CC(O...: a branch left open
    v = SmilesVocabulary(chars)
    strings = v.decode(tokens)
    assert [S.check(s)[0] for s in strings] == [32 if r == best * G2 else 0 for r in range(N2 * G2)]
    out = screen_tokens_diverse(fwd, tokens, cond, DEV, N2, K2, vocabulary=v, forward_noise=noise(), **kw)
    plain = screen_tokens(fwd, tokens, cond, DEV, N2, K2, forward_noise=noise(), **kw)
    status = out.status.cpu().numpy()
    assert status[best, 0] == 32 and int(status.sum()) == 32 and int(plain.status.sum()) == 0
    assert int(plain.index[0, 0]) == best and best not in out.index[0].tolist()
    order = [c for c in full.index[0].tolist() if c != best]
    assert out.index[0].tolist() == order[:K2] and out.index[1].tolist() == full.index[1].tolist()[:K2]
    assert out.count.tolist() == [K2, K2]
    rows = out.index.cpu() * G2 + torch.arange(G2).unsqueeze(1)
    assert torch.equal(out.tokens.cpu(), tokens[rows])
    assert torch.equal(out.score[0].cpu(), full.score[0].cpu()[[full.index[0].tolist().index(c) for c in order[:K2]]])
    assert torch.equal(out.score[1], full.score[1, :K2]) and torch.equal(out.props[1], full.props[1, :K2])
    assert float(((out.status & 96) == 0).float().mean()) == 1 - 1 / (N2 * G2)                  # the valid fraction
    # everyone malformed but one: count and tokens follow
    lone = SmilesVocabulary({C: "C", O: "O", **{20 + r: ")" for r in range(N2 * G2)}, 20 + best * G2: "N"})
    few = screen_tokens_diverse(fwd, tokens, cond, DEV, N2, K2, vocabulary=lone, forward_noise=noise(), **kw)
    assert few.count.tolist() == [1, 0] and few.index.tolist() == [[best, -1], [-1, -1]]
    assert torch.equal(few.tokens[0, 0].cpu(), tokens[best * G2]) and not few.tokens[0, 1].any() and not few.tokens[1].any()
    assert int(((few.status & 32) != 0).sum()) == N2 * G2 - 1
    # without a vocabulary: today's result, field for field
    same_call = screen_tokens_diverse(fwd, tokens, cond, DEV, N2, K2, forward_noise=noise(), **kw)
    for name in plain._fields:
        a, b = getattr(same_call, name), getattr(plain, name)
        assert a.dtype == b.dtype and torch.equal(a, b), name
