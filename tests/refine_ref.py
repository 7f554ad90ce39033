"""Host reference of mdt_refine_enter (include/mdt_hip.h; k_refine_enter in csrc/k_elem.hip), numpy only.

Contract: a row with start[b] == i gets x[b] = src[b] + sigma * n[b] (a float32 multiply, then a float32 add) and
xin[b, l, c] = c_in * x[b, c, l] for c < C, 0 for C <= c < Cp; every other row of x and xin is left as it was.  src is dense
(B, C, L) or the +-1 one-hot of draft ids (B, L).  n is the caller's tensor -- then the result is bit-exact -- or, seeded,
noise_ref.normals(seed, draw, sample0, B, C, L) in float64: the kernel deviates from that by its logf / sqrtf / sincosf error.
"""
import numpy as np

import noise_ref


def one_hot(draft, C):
    """+1 at the id's channel, -1 elsewhere: (B, L) ids -> float32 (B, C, L)."""
    return np.where(np.asarray(draft)[:, None, :] == np.arange(C)[None, :, None], np.float32(1.0), np.float32(-1.0))


def refine_enter(x, xin, start, i, sigma, c_in, src=None, draft=None, noise=None, seed=0, draw=0, sample0=0):
    """Returns (x, xin, entering) after the launch at step i.  With ``noise`` everything is float32 arithmetic in the kernel's
    order; seeded, the entering rows are float64 values from the float64 normals."""
    assert (src is None) != (draft is None)
    B, C, L = x.shape
    Cp = xin.shape[2]
    entering = np.asarray(start) == i
    s = np.asarray(src, dtype=np.float32) if src is not None else one_hot(draft, C)
    if noise is not None:
        dt = np.float32
        n = np.asarray(noise, dtype=np.float32)
    else:
        dt = np.float64
        n = noise_ref.normals(seed, draw, sample0, B, C, L)
    xo, xino = np.array(x, dtype=dt), np.array(xin, dtype=dt)
    # (the kernel takes sigma and c_in as floats)
    prod = (dt(np.float32(sigma)) * n).astype(dt)          # separate multiply ...
    xe = (s.astype(dt) + prod).astype(dt)                  # ... and add
    xine = np.zeros((B, L, Cp), dtype=dt)
    xine[:, :, :C] = (dt(np.float32(c_in)) * xe).astype(dt).transpose(0, 2, 1)
    xo[entering], xino[entering] = xe[entering], xine[entering]
    return xo, xino, entering
