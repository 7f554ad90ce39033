"""Inputs and fp64 references for the attention softmaxes of csrc/ at the edges of their range (CPU, no GPU): what
tests/test_gpu_softmax_range.py compares the kernels with and tests/test_softmax_ref_host.py checks on the host.

Every case yields three CPU tensors from ONE closed form: R (fp64), I (fp32, same expressions) and R16 (fp64 with every matrix
operand in the split-bf16 format), and from them the two reference-only error figures e_ref = max|I - R|, e16 = max|R16 - R|.
The budget of check() is built from those two figures alone."""
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

from moleculediffusiontransformer_amd import runtime as rt

H, D, F_CTX = 8, 64, 128                 # heads, head features (MDT_OP_ATTN), context features (MDT_OP_ATTN_CTX)
N_CTX, MID = 12, 512                     # context rows and attention width of the fused blocks
A, S, W = rt.SP_ACT, rt.SP_SHR, rt.SP_WEIGHT
FLOOR = 2e-6
EXP_MAX = 89.0                           # fp32 exp overflows past 88.72: no softmax that keeps the maximum in survives such a logit

Refs = namedtuple("Refs", "R I R16 e_ref e16 smax")


def ref(space, off=0):
    return rt.MdtRef(space, 0, off)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def ident(x):
    return x


def r16(x):
    """The split-bf16 operand format: hi = bf16(x), lo = bf16(x - hi); the dropped term is ~2^-18 |x|."""
    hi = x.to(torch.bfloat16).to(x.dtype)
    return hi + (x - hi).to(torch.bfloat16).to(x.dtype)


# ---- softmaxes: the right one, and the deliberately wrong ones of the host test --------------------------------------------------

def softmax(s):
    return s.softmax(-1)


def uniform(s):
    """What zero logits must give: 1 / Tk over exactly the row's own keys."""
    return torch.full_like(s, 1.0 / s.shape[-1])


def naive(s):
    """exp(s) / sum exp(s): no maximum subtracted."""
    e = s.exp()
    return e / e.sum(-1, keepdim=True)


def leaky(s):
    """One masked lane (a padded key, or a key of another sample of the tile) whose shifted logit is 0 and not -inf: weight 1 in
    the sum; its value row is zero."""
    e = (s - s.amax(-1, keepdim=True)).exp()
    return e / (e.sum(-1, keepdim=True) + 1)


def online_alpha1(s, chunk=64):
    """Online softmax over key chunks whose rescale factor is stuck at 1: every chunk's terms stay relative to the running maximum
    of ITS time."""
    run = torch.stack([c.amax(-1) for c in s.split(chunk, -1)], -1).cummax(-1).values
    w = (s - run.repeat_interleave(chunk, -1)[..., : s.shape[-1]]).exp()
    return w / w.sum(-1, keepdim=True)


# ---- closed forms ----------------------------------------------------------------------------------------------------------------

def attn_ref(q, k, v, scale, dtype=torch.float64, rr=ident, softmax=softmax):
    """softmax(q k^T scale) v per head.  q [B, T, H, D], k / v [B, Tk, H, D] -> [B, T, H, D]."""
    q_, k_, v_ = (t.to(dtype).transpose(1, 2) for t in (q, k, v))
    s = rr(q_) @ rr(k_).transpose(-1, -2) * scale
    return (rr(softmax(s)) @ rr(v_)).transpose(1, 2)


def attn_logits(q, k, scale):
    return q.double().transpose(1, 2) @ k.double().transpose(1, 2).transpose(-1, -2) * scale      # [B, H, T, Tk]


def ctx_ref(q, c, scale, dtype=torch.float64, rr=ident, softmax=softmax):
    """softmax(q c^T scale) c with keys = values = the context rows.  q [B, R, F], c [B, Tk, F] -> [B, R, F]."""
    q_, c_ = q.to(dtype), c.to(dtype)
    s = rr(q_) @ rr(c_).transpose(1, 2) * scale
    return rr(softmax(s)) @ rr(c_)


def ctx_logits(q, c, scale):
    return q.double() @ c.double().transpose(1, 2) * scale                                       # [B, R, Tk]


def _attention(h, sd, p, kv, gain, dtype, rr, softmax, logits):
    """h + Attention(h) of the reference's module: LayerNorm, to_q (times gain) / to_kv of the normalised context (or given K | V
    rows kv [B, Tk, 2 MID]), softmax, to_out."""
    def g(n):
        return sd[p + n].to(dtype)
    B, T, C = h.shape
    xn = F.layer_norm(h, (C,), g("norm.weight"), g("norm.bias"), 1e-5)
    q = (rr(xn) @ rr(g("to_q.weight") * gain).T).view(B, T, H, D).transpose(1, 2)
    if kv is None:
        cn = F.layer_norm(h, (C,), g("norm_context.weight"), g("norm_context.bias"), 1e-5)
        kv = rr(cn) @ rr(g("to_kv.weight")).T
    k, v = kv.to(dtype).chunk(2, dim=-1)
    k = k.reshape(B, -1, H, D).transpose(1, 2)
    v = v.reshape(B, -1, H, D).transpose(1, 2)
    s = rr(q) @ rr(k).transpose(-1, -2) * 0.125
    if logits is not None:
        logits.append(s)
    o = (rr(softmax(s)) @ rr(v)).transpose(1, 2).reshape(B, T, MID)
    return h + rr(o) @ rr(g("attention.to_out.weight")).T + g("attention.to_out.bias")


def subblock_ref(x, sd, prefix, mode, kv=None, gain=1.0, dtype=torch.float64, rr=ident, softmax=softmax, logits=None):
    """One attention sub-block (rt.TB_SELF / rt.TB_CROSS) on x [B, T, C]; cross blocks attend to the K | V rows kv."""
    assert (mode == rt.TB_CROSS) == (kv is not None)
    return _attention(x.to(dtype), sd, prefix, kv, gain, dtype, rr, softmax, logits)


def transformer_ref(x, sd, prefix, layers, cross, kv=None, gain=1.0, dtype=torch.float64, rr=ident, softmax=softmax, logits=None):
    """Transformer1d of the reference on x [B, T, C]: GroupNorm(32) + 1x1 to_in, per layer self-attention, cross-attention on
    kv[layer] [B, Tk, 2 MID], GELU feed-forward, then the 1x1 to_out."""
    def g(n):
        return sd[prefix + n].to(dtype)
    h = F.group_norm(x.to(dtype).transpose(1, 2), 32, g("to_in.0.weight"), g("to_in.0.bias"), 1e-6).transpose(1, 2)
    h = rr(h) @ rr(g("to_in.1.weight")[:, :, 0]).T + g("to_in.1.bias")
    for li in range(layers):
        bp = prefix + f"blocks.{li}."
        h = _attention(h, sd, bp + "attention.", None, gain, dtype, rr, softmax, logits)
        if cross:
            h = _attention(h, sd, bp + "cross_attention.", kv[li], gain, dtype, rr, softmax, logits)
        f_ = f"blocks.{li}.feed_forward."
        h = h + rr(F.gelu(rr(h) @ rr(g(f_ + "0.weight")).T + g(f_ + "0.bias"))) @ rr(g(f_ + "2.weight")).T + g(f_ + "2.bias")
    return rr(h) @ rr(g("to_out.1.weight")[:, :, 0]).T + g("to_out.1.bias")


def refs_of(form, smax):
    """R / I / R16 of one closed form `form(dtype, rr)` and the two reference-only error figures."""
    R, I, R16 = form(torch.float64, ident), form(torch.float32, ident), form(torch.float64, r16)
    return Refs(R, I, R16, (I.double() - R).abs().max().item(), (R16 - R).abs().max().item(), smax)


# ---- the budget ------------------------------------------------------------------------------------------------------------------

def budget(refs, split):
    """Exact-fp32-product paths: 8 e_ref + floor; split-bf16 paths: 8 e_ref + 4 e16 + floor; floor = 2e-6 max(1, |R|max).
    8: another summation order doubles a max statistic, the folded scale log2 e rounds a logit of magnitude 1.44 |s| once more,
    v_exp_f32 / __expf and v_rcp_f32 cost an ulp each, the branch-free erf of GELU 1.5e-7.  4: R16 rounds the operands once per
    product stage, the kernels also drop lo * lo and accumulate in fp32.  Both multiply figures of the reference alone."""
    return 8 * refs.e_ref + (4 * refs.e16 if split else 0.0) + FLOOR * max(1.0, refs.R.abs().max().item())


def ratio(G, refs, split, R=None):
    """max|G - R| / budget; inf for a non-finite G."""
    if not torch.isfinite(G).all():
        return float("inf")
    return ((G.double() - (refs.R if R is None else R)).abs().max() / budget(refs, split)).item()


def check(G, refs, split, R=None):
    r = ratio(G.reshape(refs.R.shape), refs, split, R)
    assert r <= 1.0, f"max|G - R| is {r:.3g} x the budget {budget(refs, split):.3g} (e_ref {refs.e_ref:.3g}, e16 {refs.e16:.3g})"
    return r


def cap_holds(refs, split):
    """A loose budget proves little: the margins over the reference's own errors stay under 5e-3 of the output's scale."""
    return 8 * refs.e_ref + (4 * refs.e16 if split else 0.0) <= 5e-3 * max(1.0, refs.R.abs().max().item())


def ulp32(x):
    """One fp32 ulp at |x| (the spacing above it), elementwise."""
    a = x.float().abs()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


def ulp16(x):
    """One bf16 ulp at |x|, elementwise."""
    return torch.exp2(torch.floor(torch.log2(x.double().abs().clamp_min(2.0 ** -126))) - 7)


# ---- stand-alone kernels: shapes and input families ------------------------------------------------------------------------------

# (kernel, B, T, Tk): the smallest shapes that reach each kernel -- launch_attn picks by Tk (<= 16, <= 32, <= 64 key tiles in
# registers) and takes k_attn_long past 64 queries or keys; a ragged last tile, an exactly full one, one query row
ATTN_SHAPES = [("k_attn<1>", 3, 16, 12), ("k_attn<1>", 5, 1, 16), ("k_attn<2>", 2, 17, 17), ("k_attn<2>", 3, 16, 32),
               ("k_attn<4>", 2, 17, 33), ("k_attn<4>", 2, 64, 64), ("k_attn_long", 2, 20, 65), ("k_attn_long", 2, 65, 16),
               ("k_attn_long", 2, 17, 197), ("k_attn_long", 2, 33, 128)]
ATTN_FAMILIES = ["hot", "shift", "onehot", "flat"]
# (kernel, B, T, Tk, in16, out16, merged): bf16 operands, widened exactly
ATTN16_CASES = [("k_attn<2>", 2, 32, 32, 3, 0, True), ("k_attn<2>", 2, 32, 32, 3, 1, True), ("k_attn<2>", 2, 32, 32, 2, 0, False),
                ("k_attn_long", 2, 17, 197, 3, 0, False), ("k_attn_long", 2, 17, 197, 3, 1, False)]
# k_attn_ctx<1> serves T * H <= 16 rows per sample, <2> the rest.  The launch is persistent: at most 2 workgroups per CU (2048 waves
# on 256 CUs), one unit = one sample (<1>) or one 32-row block of a sample (<2>), wave w takes units w, w + waves, ...  Only past
# 2048 units does a wave cross a unit boundary, where the running maximum and sum are reset and the previous unit is stored from
# the accumulators: B = 4200 at (1, 33) is 4200 units of <1>, B = 1100 at (16, 20) 4400 units of <2> (two or three per wave);
# B = 1100 at (4, 64) is 1100 units, one per wave, on 275 workgroups
CTX_SHAPES = [("k_attn_ctx<1>", 3, 2, 9), ("k_attn_ctx<1>", 5, 1, 33), ("k_attn_ctx<1>", 2, 2, 64), ("k_attn_ctx<1>", 4200, 1, 33),
              ("k_attn_ctx<2>", 3, 4, 20), ("k_attn_ctx<2>", 2, 16, 64), ("k_attn_ctx<2>", 1100, 4, 64),
              ("k_attn_ctx<2>", 1100, 16, 20)]
CTX_FAMILIES = ["hot", "hotter", "shift", "onehot", "flat"]


def attn_families(Tk):
    return ATTN_FAMILIES + (["stairs_up", "stairs_down"] if Tk > 64 else [])


def winners(n_rows, Tk, chunk):
    """j*(row) of the onehot family: key 0, 15, 16, Tk - 1, 63, 64 and the first key of the last chunk where they exist, then
    (7 row + 3) mod Tk."""
    listed = [j for j in (0, 15, 16, Tk - 1, 63, 64, (Tk - 1) // chunk * chunk) if 0 <= j < Tk]
    listed = list(dict.fromkeys(listed))
    assert n_rows >= len(listed)
    j = (7 * torch.arange(n_rows) + 3) % Tk
    j[: len(listed)] = torch.tensor(listed)
    return j, listed


def _bf16(x):
    return x.to(torch.bfloat16).float()


@functools.lru_cache(maxsize=None)
def attn_case(B, T, Tk, family, in16=0):
    """q [B, T, H, D], k, v [B, Tk, H, D] (fp32; bf16-representable where in16 says so), scale, the fp64 logits, and per family:
    'win' [B, T, H] the winner of every row (onehot), 'k0' the unshifted keys (shift)."""
    scale = D ** -0.5
    q = rnd(B * T * H * D, seed=1).view(B, T, H, D)
    kv = rnd(B * Tk * 2 * H * D, seed=2).view(B, Tk, 2, H, D)
    k, v = kv[:, :, 0].clone(), kv[:, :, 1].clone()
    extra = {}
    if family == "hot":
        q, k = q * 5.5, k * 5.5
    elif family == "shift":
        k[..., 63] += 150.0
        extra["k0"] = k.clone()
        extra["k0"][..., 63] -= 150.0                     # exact: the unshifted keys that k is 150 away from
        q[..., 63] = 8.0
        q[:, 1::2, :, 63] = -8.0
    elif family == "onehot":
        k = k * (8.0 / k.norm(dim=-1, keepdim=True))
        if in16 & 2:
            k = _bf16(k)
        j, listed = winners(B * H * T, Tk, 64 if Tk > 64 else 16)
        win = j.view(B, H, T).permute(0, 2, 1)                                     # row (b, h, i) -> [B, T, H]
        q = 20.0 * torch.gather(k, 1, win.unsqueeze(-1).expand(B, T, H, D))
        extra.update(win=win, listed=listed)
    elif family in ("stairs_up", "stairs_down"):
        q[..., 63] = 8.0
        k[..., 63] = (30.0 if family == "stairs_up" else -30.0) * (torch.arange(Tk) // 64).float().view(1, Tk, 1)
    elif family == "flat":
        q = torch.zeros_like(q)
    else:
        assert family == "benign"
    if in16 & 1:
        q = _bf16(q)
    if in16 & 2:
        k, v = _bf16(k), _bf16(v)
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    return dict(q=q, k=k, v=v, scale=scale, logits=attn_logits(q, k, scale), family=family, **extra)


@functools.lru_cache(maxsize=None)
def attn_refs(B, T, Tk, family, in16=0):
    c = attn_case(B, T, Tk, family, in16)
    return refs_of(lambda dt, rr: attn_ref(c["q"], c["k"], c["v"], c["scale"], dt, rr), c["logits"].abs().max().item())


@functools.lru_cache(maxsize=2)             # (the large batches: nothing is kept past the next case)
def ctx_case(B, T, Tk, family):
    """q [B, T H, F], c [B, Tk, F], scale 0.125, the fp64 logits; 'win' [B, T H] (onehot), 'c0' / 'u' (shift: c = c0 + u)."""
    R = T * H
    q = rnd(B * R * F_CTX, seed=1).view(B, R, F_CTX) * 0.3
    c = rnd(B * Tk * F_CTX, seed=2).view(B, Tk, F_CTX)
    extra = {}
    if family in ("hot", "shift"):
        q = q * 12.0                                      # logits within about +-20
    elif family == "hotter":
        q = q * 72.0                                      # +-120, as the hot family of MDT_OP_ATTN: past fp32 exp's range
    if family == "shift":
        # keys are values: a common offset u moves every logit of a row by q . u scale (+-150 here) and the output by u
        u = torch.zeros(F_CTX)
        u[127] = 40.0
        q[..., 127] = 30.0
        q[:, 1::2, 127] = -30.0
        c = c + u
        extra.update(c0=c - u, u=u)                       # exact: the context rows that c is u away from
    elif family == "onehot":
        c = c * (F_CTX ** 0.5 / c.norm(dim=-1, keepdim=True))
        j, listed = winners(B * R, Tk, 16)
        win = j.view(B, R)
        q = 8.0 * torch.gather(c, 1, win.unsqueeze(-1).expand(B, R, F_CTX))
        extra.update(win=win, listed=listed)
    elif family == "flat":
        q = torch.zeros_like(q)
    else:
        assert family in ("benign", "hot", "hotter", "shift")
    q, c = q.contiguous(), c.contiguous()
    return dict(q=q, c=c, scale=0.125, logits=ctx_logits(q, c, 0.125), family=family, **extra)


@functools.lru_cache(maxsize=2)
def ctx_refs(B, T, Tk, family):
    c = ctx_case(B, T, Tk, family)
    return refs_of(lambda dt, rr: ctx_ref(c["q"], c["c"], c["scale"], dt, rr), c["logits"].abs().max().item())


# ---- fused kernels: weights, gains, cases ----------------------------------------------------------------------------------------

GAINS = [0, 8, 32]


def subblock_sd(p, C):
    """The sub-block parameters of test_gpu_ops.test_fused_transformer_sub_block."""
    return {p + "norm.weight": 1 + 0.2 * rnd(C, seed=1), p + "norm.bias": 0.2 * rnd(C, seed=2),
            p + "norm_context.weight": 1 + 0.2 * rnd(C, seed=3), p + "norm_context.bias": 0.2 * rnd(C, seed=4),
            p + "to_q.weight": rnd(MID, C, seed=5, scale=C ** -0.5), p + "to_kv.weight": rnd(2 * MID, C, seed=6, scale=C ** -0.5),
            p + "attention.to_out.weight": rnd(C, MID, seed=7, scale=MID ** -0.5), p + "attention.to_out.bias": 0.1 * rnd(C, seed=8),
            p + "0.weight": rnd(2 * C, C, seed=9, scale=C ** -0.5), p + "0.bias": 0.1 * rnd(2 * C, seed=10),
            p + "2.weight": rnd(C, 2 * C, seed=11, scale=(2 * C) ** -0.5), p + "2.bias": 0.1 * rnd(C, seed=12)}


def transformer_sd(p, C, layers, cross, ctx=128, mid=MID, seed0=100):
    """The Transformer1d parameters of test_gpu_ops.test_fused_transformer (the reference's key names)."""
    k = [seed0]

    def r(*shape, scale=1.0):
        k[0] += 1
        return rnd(*shape, seed=k[0], scale=scale)
    sd = {p + "to_in.0.weight": 1 + 0.2 * r(C), p + "to_in.0.bias": 0.2 * r(C),
          p + "to_in.1.weight": r(C, C, 1, scale=C ** -0.5), p + "to_in.1.bias": 0.1 * r(C),
          p + "to_out.1.weight": r(C, C, 1, scale=C ** -0.5), p + "to_out.1.bias": 0.1 * r(C)}
    for li in range(layers):
        for name, cf in (("attention.", C),) + ((("cross_attention.", ctx),) if cross else ()):
            q = p + f"blocks.{li}." + name
            sd.update({q + "norm.weight": 1 + 0.2 * r(C), q + "norm.bias": 0.2 * r(C),
                       q + "norm_context.weight": 1 + 0.2 * r(cf), q + "norm_context.bias": 0.2 * r(cf),
                       q + "to_q.weight": r(mid, C, scale=C ** -0.5), q + "to_kv.weight": r(2 * mid, cf, scale=cf ** -0.5),
                       q + "attention.to_out.weight": r(C, mid, scale=mid ** -0.5), q + "attention.to_out.bias": 0.1 * r(C)})
        q = p + f"blocks.{li}.feed_forward."
        sd.update({q + "0.weight": r(2 * C, C, scale=C ** -0.5), q + "0.bias": 0.1 * r(2 * C),
                   q + "2.weight": r(C, 2 * C, scale=(2 * C) ** -0.5), q + "2.bias": 0.1 * r(C)})
    return sd


def with_gain(sd, gain):
    """sd with every to_q.weight times gain: the only handle on the logits of a fused kernel."""
    return {k: (v * float(gain) if k.endswith("to_q.weight") else v) for k, v in sd.items()}


# (kernel, variant, mode, C, T, B): variant 0 = k_tblock_lw (C = 128, cross blocks with at most 16 keys per 16-row tile, which
# rules out cross at T = 4 with 12 context rows), 2 / 3 / 4 = k_tblock32 (C = 256; 4 = chained input, split partial sums)
TBLOCK_CASES = ([("k_tblock_lw", 0, m, 128, T, B) for m, T, B in ((rt.TB_SELF, 16, 5), (rt.TB_SELF, 4, 16), (rt.TB_CROSS, 16, 5))]
                + [("k_tblock32", var, m, 256, T, B) for var in (2, 3, 4) for m in (rt.TB_SELF, rt.TB_CROSS)
                   for T, B in ((4, 37), (16, 3))])
# (kernel, C, T, B, layers, cross, gains): two layers at gain 8 only -- peaky attention amplifies rounding through a second
# layer (e16 = 9e-3 at gain 32), and a budget that wide proves little
TF_CASES = [("k_tf128", 128, 16, 5, 1, False, GAINS), ("k_tf128", 128, 4, 16, 1, False, GAINS),
            ("k_tf128", 128, 16, 3, 1, True, GAINS), ("k_tf128", 128, 16, 5, 2, False, [8]),
            ("k_tf256", 256, 4, 5, 1, True, GAINS), ("k_tf256", 256, 16, 3, 1, False, GAINS),
            ("k_tf256", 256, 4, 37, 2, True, [8])]


@functools.lru_cache(maxsize=None)
def tblock_case(variant, mode, C, T, B):
    p = "blk."
    n_x, n_kv = T * C, N_CTX * 2 * MID
    x, kv = rnd(B * n_x, seed=13) * 1.5 + 0.3, rnd(B * n_kv, seed=14)
    p_in = 0.5 * rnd(B * n_x, seed=15) if variant == 4 else None
    return dict(p=p, sd=subblock_sd(p, C), x=x, kv=kv, p_in=p_in, variant=variant, mode=mode, C=C, T=T, B=B)


def tblock_form(c, gain, softmax=softmax, logits=None):
    """The closed form of a sub-block case as form(dtype, rr)."""
    B, T, C = c["B"], c["T"], c["C"]
    x = c["x"].view(B, T, C)
    kv = c["kv"].view(B, N_CTX, 2 * MID) if c["mode"] == rt.TB_CROSS else None

    def form(dt, rr):
        x_in = x.to(dt) if c["p_in"] is None else x.to(dt) + c["p_in"].view(B, T, C).to(dt)
        return subblock_ref(x_in, c["sd"], c["p"], c["mode"], kv, gain, dt, rr, softmax,
                            logits if dt == torch.float64 and rr is ident else None)
    return form


@functools.lru_cache(maxsize=None)
def tblock_refs(variant, mode, C, T, B, gain):
    logits = []
    form = tblock_form(tblock_case(variant, mode, C, T, B), gain, logits=logits)
    R = refs_of(form, 0.0)
    return R._replace(smax=max(s.abs().max().item() for s in logits))


@functools.lru_cache(maxsize=None)
def tf_case(C, T, B, layers, cross):
    p = "tf."
    kv_floats = N_CTX * 2 * MID
    x = rnd(B * T * C, seed=13) * 1.5 + 0.3
    kv = rnd(layers * B * kv_floats, seed=14) if cross else torch.zeros(0)
    return dict(p=p, sd=transformer_sd(p, C, layers, cross), x=x, kv=kv, C=C, T=T, B=B, layers=layers, cross=cross)


def tf_form(c, gain, softmax=softmax, logits=None):
    B, T, C = c["B"], c["T"], c["C"]
    kv = c["kv"].view(c["layers"], B, N_CTX, 2 * MID) if c["cross"] else None

    def form(dt, rr):
        return transformer_ref(c["x"].view(B, T, C), c["sd"], c["p"], c["layers"], c["cross"], kv, gain, dt, rr, softmax,
                               logits if dt == torch.float64 and rr is ident else None)
    return form


@functools.lru_cache(maxsize=None)
def tf_refs(C, T, B, layers, cross, gain):
    logits = []
    R = refs_of(tf_form(tf_case(C, T, B, layers, cross), gain, logits=logits), 0.0)
    return R._replace(smax=max(s.abs().max().item() for s in logits))


# ---- lowering: the ops of test_gpu_ops.py, built the same way -------------------------------------------------------------------
# Each returns (ops, weights, act, shr, ext, B, out, untouched): out(act') = the op's result in the shape of R, untouched = the
# [lo, hi) ranges of act that hold inputs.

def _pack16(x, half):
    return x.to(torch.bfloat16).view(torch.float32) if half else x


def lower_attn(c, in16=0, out16=0, merged=False):
    q, k, v = c["q"], c["k"], c["v"]
    B, T = q.shape[:2]
    Tk = k.shape[1]
    kv = torch.stack([k, v], 2)                                                   # [B, Tk, 2, H, D]
    if merged:
        assert in16 == 3 and T == Tk
        regions = [_pack16(torch.cat([q.reshape(B * T, H * D), kv.reshape(B * Tk, 2 * H * D)], 1).reshape(-1), True)]
    else:
        regions = [_pack16(q.reshape(-1), in16 & 1), _pack16(kv.reshape(-1), in16 & 2)]
    n_in = sum(r.numel() for r in regions)
    act = torch.cat(regions + [torch.zeros(B * T * H * D // (2 if out16 else 1))])
    op = rt.MdtOp()
    op.kind = rt.OP_ATTN
    op.a, op.out = ref(A, 0), ref(A, n_in // B)
    i = op.i
    if merged:
        op.a2 = ref(A, 0)
        i[rt.A_LDQ], i[rt.A_LDKV], i[rt.A_KCOL] = 3 * H * D, 3 * H * D, H * D
    else:
        op.a2 = ref(A, regions[0].numel() // B)
        i[rt.A_LDQ], i[rt.A_LDKV] = H * D, 2 * H * D
    i[rt.A_T], i[rt.A_TK], i[rt.A_HEADS], i[rt.A_LDO], i[rt.A_KV_BSTRIDE] = T, Tk, H, H * D, Tk
    i[rt.A_IN16], i[rt.A_OUT16] = in16, out16
    op.f[0] = c["scale"]

    def out(a):
        o = a[n_in:]
        return (o.view(torch.bfloat16).float() if out16 else o).view(B, T, H, D)
    return [op], torch.zeros(4), act, torch.zeros(4), {}, B, out, [(0, n_in)]


def lower_ctx(c, T, split):
    q, cx = c["q"], c["c"]
    B, R = q.shape[:2]
    Tk = cx.shape[1]
    act = torch.cat([q.reshape(-1), cx.reshape(-1), torch.zeros(B * R * F_CTX)])
    n_in = B * (R + Tk) * F_CTX
    op = rt.MdtOp()
    op.kind = rt.OP_ATTN_CTX
    op.a, op.out, op.a2 = ref(A, 0), ref(A, R * F_CTX + Tk * F_CTX), ref(A, R * F_CTX)
    i = op.i
    i[rt.A_T], i[rt.A_TK], i[rt.A_HEADS], i[rt.A_LDQ], i[rt.A_LDKV], i[rt.A_LDO] = T, Tk, H, F_CTX, F_CTX, F_CTX
    i[rt.A_KV_BSTRIDE] = Tk
    i[rt.A_SPLIT] = split
    op.f[0] = c["scale"]
    return [op], torch.zeros(4), act, torch.zeros(4), {}, B, (lambda a: a[n_in:].view(B, R, F_CTX)), [(0, n_in)]


def _cfg():
    from moleculediffusiontransformer_amd.netspec import inverse_unet_config
    return inverse_unet_config(16, 64, 128, N_CTX)


def lower_tblock(c, gain, prod):
    """MDT_OP_TBLOCK as test_fused_transformer_sub_block (variants 0 / 2 / 3: in place on x, K | V rows behind it, variant 3's
    partial-sum scratch behind those) and test_chained_split_sub_block (variant 4: x + p_in -> x_out and the second head
    group's bare partial sum in p_out; the block's result is their sum)."""
    from moleculediffusiontransformer_amd.compiler import Ten, UNetCompiler
    variant, mode, C, T, B = c["variant"], c["mode"], c["C"], c["T"], c["B"]
    comp = UNetCompiler(_cfg(), 64, N_CTX, with_gain(c["sd"], gain), gemm_mode=prod)
    n_x, n_kv = T * C, N_CTX * 2 * MID
    cross_index = 0 if mode == rt.TB_CROSS else None
    if variant == 4:
        x_out, p_in, p_out = Ten(A, n_x + n_kv, T, C), Ten(A, 2 * n_x + n_kv, T, C), Ten(A, 3 * n_x + n_kv, T, C)
        comp.tblock(Ten(A, 0, T, C), mode, c["p"], cross_index, variant=4, x_out=x_out, p_in=p_in, p_out=p_out)
        act = torch.cat([c["x"], c["kv"], torch.zeros(B * n_x), c["p_in"], torch.zeros(B * n_x)])
        lo = B * (n_x + n_kv)

        def out(a):
            return (a[lo: lo + B * n_x] + a[lo + 2 * B * n_x:]).view(B, T, C)
        untouched = [(0, lo), (lo + B * n_x, lo + 2 * B * n_x)]
    else:
        comp.tblock(Ten(A, 0, T, C), mode, c["p"], cross_index, variant=variant)
        act = torch.cat([c["x"], c["kv"]])
        if variant == 3:
            comp.ops[0].out = ref(A, n_x + n_kv)
            act = torch.cat([act, torch.zeros(B * 2 * n_x)])

        def out(a):
            return a[: B * n_x].view(B, T, C)
        untouched = [(B * n_x, B * (n_x + n_kv))]
    op = comp.ops[0]
    assert op.kind == rt.OP_TBLOCK and op.i[rt.B_WF32] == int(prod == "f32") and op.i[rt.B_VARIANT] == variant
    if mode == rt.TB_CROSS:
        op.a2 = ref(A, n_x)
    return [op], comp.W.pack(), act, torch.zeros(4), {}, B, out, untouched


def handoff_ext(B, T):
    """bindings.ext[3] / [4] of a pair-split MDT_OP_TF256: zeroed flag words, hand-off blocks."""
    nrb = (B * T + 31) // 32
    return {3: torch.zeros(64 + 64 * nrb), 4: torch.zeros(2 * nrb * 2 * 32 * 256)}


def lower_tf(c, gain, prod, form="whole"):
    """MDT_OP_TF128 / MDT_OP_TF256 as test_fused_transformer: per-sample arena [x | y | K/V layer 0 | K/V layer 1 ...]."""
    from moleculediffusiontransformer_amd.compiler import Ten, UNetCompiler
    C, T, B, layers, cross = c["C"], c["T"], c["B"], c["layers"], c["cross"]
    comp = UNetCompiler(_cfg(), 64, N_CTX, with_gain(c["sd"], gain), gemm_mode=prod, tf256=(form == "whole"))
    comp.pair_stride = 1 if form == "pair1" else 8
    assert comp.tf128_ok(C, T, layers, cross) or comp.tf256_ok(C, T, layers, cross)
    comp.transformer(Ten(A, 0, T, C), c["p"], C, layers, cross, free_input=False)
    assert [o.kind for o in comp.ops] == [rt.OP_TF128 if C == 128 else rt.OP_TF256]
    op = comp.ops[0]
    assert op.i[rt.F_WF32] == int(prod == "f32")
    assert op.i[rt.F_NSPLIT] == (2 if (C == 256 and form != "whole") else (1 if C == 256 else 0))
    op.out = ref(A, T * C)
    if cross:
        op.a2 = ref(A, 2 * T * C)
    act = torch.cat([c["x"], torch.zeros(B * T * C), c["kv"]])
    ext = handoff_ext(B, T) if form != "whole" else {}
    n = B * T * C
    return [op], comp.W.pack(), act, torch.zeros(4), ext, B, (lambda a: a[n: 2 * n].view(B, T, C)), [(0, n), (2 * n, act.numel())]
