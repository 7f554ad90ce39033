"""numpy-only reference of the screening kernels (csrc/k_screen.hip) and of the host key: plain loops written from the contract
in include/mdt_hip.h, sharing no code with the package."""
import numpy as np

EMPTY, NONFINITE, DUPLICATE, KNOWN = 1, 2, 4, 8
MASK = (1 << 64) - 1


def mix(x):
    """One splitmix64 step on a Python int."""
    z = (x + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def row_key(ids):
    """Key of an already compacted list of ids."""
    k = 0
    for j, t in enumerate(ids):
        k = (k + mix((j << 32) | (int(t) & 0xFFFFFFFF))) & MASK
    return k


def compact(tokens, Lf=0, x_norm=1.0):
    """-> (packed int32 (B, L), length int32 (B), key uint64 (B), fwd_in float32 (B, Lf))."""
    tokens = np.asarray(tokens)
    B, L = tokens.shape
    packed, length = np.zeros((B, L), np.int32), np.zeros(B, np.int32)
    key, fwd = np.zeros(B, np.uint64), np.zeros((B, Lf), np.float32)
    for b in range(B):
        ids = [int(t) for t in tokens[b] if int(t) != 0]
        packed[b, :len(ids)] = ids
        length[b] = len(ids)
        key[b] = row_key(ids)
        for j, t in enumerate(ids[:Lf]):
            fwd[b, j] = np.float32(np.float64(t) / np.float64(x_norm))
    return packed, length, key, fwd


def score(props, target, weights, N):
    """props (N * G, stride >= n) fp32, target (G, n) -> fp32 (N * G): i ascending, separate fp32 multiply and add."""
    props, target = np.asarray(props, np.float32), np.asarray(target, np.float32)
    G, n = target.shape
    out = np.zeros(N * G, np.float32)
    with np.errstate(all="ignore"):
        for r in range(N * G):
            acc = np.float32(0)
            for i in range(n):
                d = np.float32(props[r, i] - target[r % G, i])
                sq = np.float32(d * d)
                if weights is not None:
                    sq = np.float32(np.float32(weights[i]) * sq)
                acc = np.float32(acc + sq)
            out[r] = np.float32(acc / np.float32(n))
    return out


def select(score_, packed, length, N, G, K, known=()):
    """Equality on the compacted rows themselves (no key): ``known`` is any iterable of compacted id tuples.
    -> (status uint8 (N * G), index int32 (G, K), count int32 (G))."""
    known = {tuple(int(t) for t in k) for k in known}
    status = np.zeros(N * G, np.uint8)
    index, count = np.full((G, K), -1, np.int32), np.zeros(G, np.int32)
    for g in range(G):
        seen, eligible = set(), []
        for c in range(N):
            r = c * G + g
            mol = tuple(int(t) for t in packed[r, :length[r]])
            st = 0
            if not mol:
                st |= EMPTY
            if not np.isfinite(score_[r]):
                st |= NONFINITE
            if mol in seen:
                st |= DUPLICATE
            if mol in known:
                st |= KNOWN
            seen.add(mol)
            status[r] = st
            if st == 0:
                eligible.append((float(score_[r]), c))
        best = sorted(eligible)[:K]
        count[g] = len(best)
        for k, (_, c) in enumerate(best):
            index[g, k] = c
    return status, index, count


def screen(tokens, props, target, N, K, weights=None, known=()):
    """The whole of screen_tokens after the forward model, on the host: -> dict of the Screened fields."""
    tokens, props, target = np.asarray(tokens), np.asarray(props, np.float32), np.asarray(target, np.float32)
    G, n = target.shape
    packed, length, _, _ = compact(tokens)
    sc = score(props, target, weights, N)
    known = [tuple(int(t) for t in row if int(t) != 0) for row in known]
    status, index, count = select(sc, packed, length, N, G, K, known)
    L = tokens.shape[1]
    out_t, out_p = np.zeros((G, K, L), np.int64), np.full((G, K, n), np.nan, np.float32)
    out_s = np.full((G, K), np.inf, np.float32)
    for g in range(G):
        for k in range(count[g]):
            r = index[g, k] * G + g
            out_t[g, k], out_p[g, k], out_s[g, k] = tokens[r], props[r, :n], sc[r]
    return dict(tokens=out_t, props=out_p, score=out_s, index=index.astype(np.int64), count=count.astype(np.int64),
                status=status.reshape(N, G))
