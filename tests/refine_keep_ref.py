"""Host reference of mdt_refine_keep_enter (include/mdt_hip.h; k_refine_keep_enter in csrc/k_elem.hip) and of the merges of the
masked refine loop (diffusion.run_refine with ``keep``), numpy only.

Contract of the launch in front of step i, per row b:

    start[b] >  i:  x[b] and xin[b] are left as they were;
    start[b] == i:  x[b] = keep ? src + sigma * n_src : src + sigma * n_entry
    start[b] <  i:  x[b] = keep ? src + sigma * n_src : x[b]

(a float32 multiply, then a float32 add: no fused multiply-add), and for the rows that run xin[b, l, c] = c_in * x[b, c, l] for
c < C, 0 for C <= c < Cp.  src is dense (B, C, L) or the +-1 one-hot of draft ids (B, L); keep is (B, C, L), or (B, L) broadcast
over the channels.  n_entry / n_src are the caller's tensors -- then the result is bit-exact -- or, seeded,
noise_ref.normals(seed, draw, sample0, B, C, L) in float64: the kernel deviates from that by its logf / sqrtf / sincosf error.
"""
import numpy as np

import noise_ref
from refine_ref import one_hot


def full_keep(keep, C):
    """keep as bool (B, C, L): a (B, L) mask is broadcast over the channels."""
    k = np.asarray(keep).astype(bool)
    return np.repeat(k[:, None, :], C, axis=1) if k.ndim == 2 else k


def keep_enter(x, xin, start, i, sigma, c_in, keep, src=None, draft=None, n_entry=None, n_src=None, seed=0, draw_entry=0,
               draw_src=0, sample0=0):
    """Returns (x, xin, runs) after the launch at step i; runs[b] = start[b] <= i.  With both noises given everything is float32
    arithmetic in the kernel's order; a noise that is None comes from the float64 normals and the result is float64."""
    assert (src is None) != (draft is None)
    B, C, L = x.shape
    Cp = xin.shape[2]
    start = np.asarray(start)
    runs, entering = start <= i, start == i
    dt = np.float32 if (n_entry is not None and n_src is not None) else np.float64
    s = (np.asarray(src, dtype=np.float32) if src is not None else one_hot(draft, C)).astype(dt)
    ne = np.asarray(n_entry, dtype=np.float32) if n_entry is not None else noise_ref.normals(seed, draw_entry, sample0, B, C, L)
    ns = np.asarray(n_src, dtype=np.float32) if n_src is not None else noise_ref.normals(seed, draw_src, sample0, B, C, L)
    k = full_keep(keep, C)
    sg = dt(np.float32(sigma))                             # (the kernel takes sigma and c_in as floats)
    noised = lambda n: (s + (sg * n.astype(dt)).astype(dt)).astype(dt)       # noqa: E731  separate multiply and add
    xo, xino = np.array(x, dtype=dt), np.array(xin, dtype=dt)
    free = np.where(entering[:, None, None], noised(ne), xo)
    xn = np.where(k, noised(ns), free).astype(dt)
    xinn = np.zeros((B, L, Cp), dtype=dt)
    xinn[:, :, :C] = (dt(np.float32(c_in)) * xn).astype(dt).transpose(0, 2, 1)
    xo[runs], xino[runs] = xn[runs], xinn[runs]
    return xo, xino, runs


def finish(x, keep, src=None, draft=None):
    """The loop's last merge and decode (mdt_inpaint_finish): x = keep ? src : x; tokens = argmax over the channels (first maximum) --
    with draft ids and a (B, L) keep, the draft id at a kept position."""
    assert (src is None) != (draft is None)
    B, C, L = x.shape
    s = np.asarray(src, dtype=np.float32) if src is not None else one_hot(draft, C)
    out = np.where(full_keep(keep, C), s, np.asarray(x, dtype=np.float32))
    tokens = out.argmax(axis=1)
    if draft is not None and np.asarray(keep).ndim == 2:
        tokens = np.where(np.asarray(keep).astype(bool), np.asarray(draft), tokens)
    return out, tokens
