"""Host references of csrc/k_elem.hip's dynamic threshold and embeddings (numpy / torch on the CPU, no GPU): what
tests/test_gpu_elem.py compares the kernels with, and tests/test_elem_ref_host.py checks against torch.quantile."""
import math

import numpy as np
import torch

from gpu_util import rnd

# (C, L, Cp): N = C * L values per sample -- the smallest, the suite's earlier size, a power of two (no padding of the sort),
# just past one (992 pads of +inf), a size whose fp32 rank can be integral, the largest the kernel accepts
DYN_SHAPES = [(1, 4, 16), (22, 32, 32), (16, 64, 16), (33, 32, 48), (3, 684, 16), (16, 2048, 16)]
DYN_QS = [0.001, 0.5, 0.9, 0.995, 1.0]
Q_INTEGRAL = 1000.0 / 2051.0            # at N = 2052: fp32(q) * fp32(N - 1) == 1000.0 exactly (asserted where it is used)
# (c_skip, c_out) of the four samples of mdt_dyn_scale_rows; the shared-coefficient kernel runs once with each of the first three
DYN_COEF = [(0.31, 0.095), (0.9, 0.05), (0.5, 0.25), (1.0, 0.0)]


def dyn_inputs(C, L, Cp):
    """x (4, C, L), pred (4, L, Cp): a Gaussian x 3 sample, one with every |v| < 1 (the scale floors at exactly 1), one quantised to
    multiples of 0.25 (heavy ties under the power-of-two coefficients (0.5, 0.25) and (1, 0)), one of all-equal values."""
    x, pred = rnd(4, C, L, seed=21) * 3, rnd(4, L, Cp, seed=22) * 3
    x[1], pred[1] = x[1].clamp(-3, 3) * 0.25, pred[1].clamp(-3, 3) * 0.25
    x[2], pred[2] = (x[2] * 4).round() / 4, (pred[2] * 4).round() / 4
    x[3], pred[3] = 2.5, -0.5
    return x.contiguous(), pred.contiguous()


def magnitudes(x, pred, c_skip, c_out):
    """|c_skip * x + c_out * pred| of one sample in float32 without contraction.  x (C, L), pred (L, Cp) torch fp32 -> numpy (N,)."""
    C = x.shape[0]
    xs, ps = x.numpy(), pred[:, :C].t().contiguous().numpy()
    v = np.float32(c_skip) * xs + np.float32(c_out) * ps
    assert v.dtype == np.float32
    return np.abs(v).reshape(-1)


def quantile_lerp(v, q):
    """torch.quantile's linear interpolation of the sorted float32 vector v at q, on np.float32 scalars (no FMA): rank = q (N - 1),
    ATen's two-sided lerp -- dyn_scale_sample's arithmetic, operation for operation."""
    s = np.sort(v.astype(np.float32))
    rank = np.float32(q) * np.float32(s.size - 1)
    below, above = np.floor(rank), np.ceil(rank)
    w = np.float32(rank - below)
    v0, v1 = s[int(below)], s[int(above)]
    diff = np.float32(v1 - v0)
    if abs(w) < np.float32(0.5):
        return np.float32(v0 + np.float32(w * diff))
    return np.float32(v1 - np.float32(diff * np.float32(np.float32(1.0) - w)))


def dyn_scale_ref(x, pred, c_skip, c_out, q):
    """max(quantile(|c_skip x + c_out pred|, q), 1) per sample.  c_skip / c_out: floats, or one per sample.  Returns float32 (B,)."""
    B = x.shape[0]
    cs = [float(c) for c in (c_skip if hasattr(c_skip, "__len__") else [c_skip] * B)]
    co = [float(c) for c in (c_out if hasattr(c_out, "__len__") else [c_out] * B)]
    return torch.tensor([max(quantile_lerp(magnitudes(x[b], pred[b], cs[b], co[b]), q), np.float32(1.0)) for b in range(B)],
                        dtype=torch.float32)


def inv_freq(D2):
    """PositionalEncoding1D's frequencies: 1 / 10000^(2j / D2), j < D2 / 2."""
    return 1.0 / (10000 ** (torch.arange(0, D2, 2).float() / D2))


def cond_embed_ref(seq, w, bias, freq, D2, add):
    """k_cond_embed in float64 on the kernel's fp32 intermediates: h = seq * w + bias and the angle pos * freq are formed in fp32
    (separate multiply and add), erf / sin / cos are evaluated in float64.  seq (B, n), w / bias (D1,), freq (D2 / 2,).
    Returns float64 (B, n, D1 + D2), or (B, n, D1) with add (the first D1 columns of [sin | cos] added to the gelu)."""
    B, n = seq.shape
    D1, half = w.numel(), D2 // 2
    h = (seq.view(B, n, 1) * w.view(1, 1, D1) + bias.view(1, 1, D1)).double()
    gelu = 0.5 * h * (1.0 + torch.erf(h * 0.70710678118654752440))
    ang = (torch.arange(n).float().view(n, 1) * freq.view(1, half)).double()
    pe = torch.cat([ang.sin(), ang.cos()], dim=1).view(1, n, D2).expand(B, -1, -1)
    if add:
        return gelu + pe[:, :, :D1]
    return torch.cat([gelu, pe], dim=2)


def time_embed_ref(t, w, ld):
    """k_time_embed: [t, sin(fr), cos(fr), 0 ...] with fr = ((t * w) * 2) * pi formed in fp32 in that order, sin / cos in float64."""
    tn, wn = t.numpy().astype(np.float32).reshape(-1, 1), w.numpy().astype(np.float32).reshape(1, -1)
    fr = ((tn * wn) * np.float32(2.0)) * np.float32(3.14159265358979323846)
    assert fr.dtype == np.float32
    fr = torch.from_numpy(fr.astype(np.float64))
    out = torch.zeros(t.numel(), ld, dtype=torch.float64)
    half = w.numel()
    out[:, 0] = t.double()
    out[:, 1: 1 + half], out[:, 1 + half: 1 + 2 * half] = fr.sin(), fr.cos()
    return out
