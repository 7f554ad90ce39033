"""numpy-only reference of the edit-distance kernels (csrc/k_edit.hip) and of mdt_screen_select_diverse (csrc/k_screen.hip): the
textbook dynamic programme, a brute-force nearest and the greedy selection as plain loops, written from the contract in
include/mdt_hip.h on top of screen_ref's status rules.  Shares no code with the package."""
import numpy as np

import screen_ref as R

CLOSE = 16


def distance(a, b):
    """Levenshtein distance of two id sequences: the two-row dynamic programme."""
    a, b = [int(t) for t in a], [int(t) for t in b]
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i] + [0] * len(b)
        for j, y in enumerate(b, 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y))
        prev = cur
    return prev[len(b)]


def distances(A, la, B, lb):
    """The same programme for P pairs at once: A, B (P, L) left-packed rows, la, lb (P) their lengths -> int32 (P)."""
    A, B, la, lb = np.asarray(A), np.asarray(B), np.asarray(la), np.asarray(lb)
    P, L = A.shape
    at = np.arange(P)
    prev = np.tile(np.arange(L + 1), (P, 1))
    out = np.where(la == 0, lb, 0)
    for i in range(1, L + 1):
        cur = np.empty_like(prev)
        cur[:, 0] = i
        for j in range(1, L + 1):
            cur[:, j] = np.minimum(np.minimum(prev[:, j] + 1, cur[:, j - 1] + 1), prev[:, j - 1] + (A[:, i - 1] != B[:, j - 1]))
        out = np.where(la == i, cur[at, lb], out)
        prev = cur
    return out.astype(np.int32)


def nearest(Q, lq, K, lk):
    """Brute force: per query row the smallest distance to a known row and the lowest index that attains it -> int32 (R), (R)."""
    Q, K = np.asarray(Q), np.asarray(K)
    Rn, M = len(Q), len(K)
    d = distances(np.repeat(Q, M, axis=0), np.repeat(lq, M), np.tile(K, (Rn, 1)), np.tile(lk, Rn)).reshape(Rn, M)
    return d.min(axis=1).astype(np.int32), d.argmin(axis=1).astype(np.int32)       # argmin: the first of equal values


def select_diverse(score, packed, length, N, G, K, known=(), known_dist=None, min_novelty=1, min_distance=1):
    """-> (status uint8 (N * G), index int32 (G, K), count int32 (G)) of mdt_screen_select_diverse."""
    status, _, _ = R.select(score, packed, length, N, G, K, known)
    if known_dist is not None:
        status = status | np.where(np.asarray(known_dist) < min_novelty, R.KNOWN, 0).astype(np.uint8)
    index, count = np.full((G, K), -1, np.int32), np.zeros(G, np.int32)
    for g in range(G):
        order = sorted((float(score[c * G + g]), c) for c in range(N) if status[c * G + g] == 0)
        kept = []
        for _, c in order:
            r = c * G + g
            close = False
            if kept:
                rows = [o * G + g for o in kept]
                d = distances(np.tile(packed[r], (len(rows), 1)), np.full(len(rows), length[r]), packed[rows], length[rows])
                close = bool((d < min_distance).any())
            if close:
                status[r] |= CLOSE
            elif len(kept) < K:
                kept.append(c)
        index[g, :len(kept)] = kept
        count[g] = len(kept)
    return status, index, count


def screen(tokens, props, target, N, K, weights=None, known=(), min_distance=1, min_novelty=1):
    """screen_tokens_diverse after the forward model, on the host: -> dict of the Screened fields.  ``known``: raw id rows."""
    tokens, props, target = np.asarray(tokens), np.asarray(props, np.float32), np.asarray(target, np.float32)
    G, n = target.shape
    packed, length, _, _ = R.compact(tokens)
    sc = R.score(props, target, weights, N)
    known_dist, exact = None, [tuple(int(t) for t in row if int(t) != 0) for row in known]
    if min_novelty > 1:
        kp, kl, _, _ = R.compact(np.asarray(known))
        wide = np.zeros((len(kp), max(kp.shape[1], packed.shape[1])), np.int32)
        wide[:, :kp.shape[1]] = kp
        keep = kl <= packed.shape[1]                                          # a longer known row equals no generated molecule
        known_dist, exact = nearest(packed, length, wide[keep][:, :packed.shape[1]], kl[keep])[0], ()
    status, index, count = select_diverse(sc, packed, length, N, G, K, exact, known_dist, min_novelty, min_distance)
    L = tokens.shape[1]
    out_t, out_p = np.zeros((G, K, L), np.int64), np.full((G, K, n), np.nan, np.float32)
    out_s = np.full((G, K), np.inf, np.float32)
    for g in range(G):
        for k in range(count[g]):
            r = index[g, k] * G + g
            out_t[g, k], out_p[g, k], out_s[g, k] = tokens[r], props[r, :n], sc[r]
    return dict(tokens=out_t, props=out_p, score=out_s, index=index.astype(np.int64), count=count.astype(np.int64),
                status=status.reshape(N, G))
