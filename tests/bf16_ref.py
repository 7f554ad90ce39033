"""The plain-bf16 mode (gemm_mode = 'bf16') held to its rounding points, per element.

The criterion, stated once.  Every op of the mode is evaluated twice on exactly the operand bits it read, bf16 operands widened
exactly (reference()):

  r  the op's documented arithmetic (include/mdt_hip.h) in fp64, rounded to bf16 only where the header says a value is stored or
     consumed as bf16 -- the A operand of MDT_G_WFMT 1 after its prologue; a bf16 OUTPUT is r before its store;
  i  the same form in fp32 with torch on the CPU; for MDT_G_WFMT 134 the kernel's own formula, rstd (A W^T - mean colsum) + bias
     with the one-pass variance q / cin - mean^2, so that e_ref carries that formula's cancellation.

  e_ref = max|i - r|;   delta = 8 e_ref + 2e-6 max(1, |r|max)      (softmax_ref.budget() on an exact-product path: the 8 covers
                                                                    another summation order, the floor the A&S erf, __expf, v_rcp_f32)
  bf16 output element   |G - r| <= ulp_bf16(r) / 2 + delta,  ulp_bf16(r) = 2^(floor(log2 |r|) - 7): the spacing of r's OWN binade
  fp32 output element   |G - r| <= delta
  bf16 copy of an fp32 tensor   bit-equal to round-to-nearest-even of the source (rne_bits: integer arithmetic on the fp32 bits)
  and every output is finite, every element of the arena that is not an output element of the op comes back bit for bit (inputs,
  the columns beside a column block, the tensors of the other ops).

Chains run one op per program (stepwise): the r of op k is computed from what the runner left in the arena before op k, so a
rounding tie in a hidden tensor cannot leak into the next op's comparison, and an in-place op is compared with its own input.

One rounding is hidden INSIDE an op: MDT_G_WFMT 1 rounds A to bf16 after its prologue.  A prologue value within a few fp32 ulps of
a bf16 rounding boundary may legitimately go either way, which moves an output by ulp_bf16(a) |w| -- far more than delta.  The
criterion is not widened for that: settle() moves such inputs (by 3e-5 of themselves) until no prologue value of the case lies
within TIE_GUARD of a boundary, so that r, i and any correct kernel round every A element the same way.

Cases are plain data (Case); runner(ops, weights, act, shr, B) -> act runs ONE op: the GPU (tests/test_gpu_bf16_elementwise.py)
or oracle/program_interp.py (tests/test_bf16_ref_host.py)."""
import math
from collections import namedtuple

import torch

from gpu_util import ref, rnd
from moleculediffusiontransformer_amd import runtime as rt

W, A, S = rt.SP_WEIGHT, rt.SP_ACT, rt.SP_SHR
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
FLOOR = 2e-6
TIE_GUARD = 2e-6          # fp32 prologue arithmetic on values of magnitude <= 8: a few ulps, 5e-7; four times that
CAP = 1e-4                # (c): a case whose references alone disagree by more than this of the scale says nothing about the kernel

# key: unique name; site: row of the table in DESIGN.md 4.3; ops: MdtOp list; check: indices of the ops held to the criterion
# (a MDT_OP_GN_STATS in front of a prologue only runs); tile / w16: mdt_set_tuning values (None = leave); planted: what the case
# plants in a copied source ("ties" ...), for the tests that count them
Case = namedtuple("Case", "key site ops weights act shr B check tile w16 planted")
# one output tensor of an op.  kind "bf16" | "f32" | "copy"; idx: element indices into the arena (bf16 units for bf16 / copy, floats
# for f32); r, i: the references (None for a copy); bits: the expected int16 patterns of a copy
# src: a copy of a tensor the op itself stored (MDT_G_WFMT 10) -- the float indices of that tensor, bits are taken from the arena after the op
Out = namedtuple("Out", "name kind idx r i bits src", defaults=(None,))


def gemm_op(**kw):
    from test_gpu_ops import gemm_op as g
    return g(**kw)


# ---- number formats ------------------------------------------------------------------------------------------------------------

def rne_bits(x):
    """Round-to-nearest-even of fp32 values to bf16, by integer arithmetic on the bits (finite inputs): int32 patterns 0..65535."""
    u = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF


def bits16(t16):
    return t16.contiguous().view(torch.int16).to(torch.int64) & 0xFFFF


def pack16(t16):
    """bf16 tensor -> the floats that hold it in the arena."""
    return t16.contiguous().view(-1).view(F32)


def ulp_bf16(r):
    """The spacing of bf16 numbers in r's own binade, elementwise (fp64)."""
    return torch.exp2(torch.floor(torch.log2(r.double().abs().clamp_min(2.0 ** -126))) - 7)


def delta(r, i):
    e_ref = (i.double() - r).abs().max().item()
    return 8 * e_ref + FLOOR * max(1.0, r.abs().max().item())


def excess(G, out, d):
    """(|G - r| - ulp / 2) / delta per element (the ulp term dropped for an fp32 output)."""
    err = (G.double() - out.r).abs()
    if out.kind == "bf16":
        err = err - 0.5 * ulp_bf16(out.r)
    return err / d


def ratio(G, out):
    if not torch.isfinite(G).all():
        return float("inf")
    return excess(G, out, delta(out.r, out.i)).max().item()


def check(G, out):
    """The assertion of the criterion on one output tensor; returns its ratio (copies: 0.0)."""
    assert torch.isfinite(G.float()).all(), f"{out.name}: a non-finite output"
    if out.kind == "copy":
        got = bits16(G)
        bad = (got != out.bits).nonzero().view(-1)
        assert bad.numel() == 0, (f"{out.name}: {bad.numel()} elements are not round-to-nearest-even of their source, first at "
                                  f"{bad[0].item()}: {got[bad[0]].item():#06x} for {out.bits[bad[0]].item():#06x}")
        return 0.0
    d = delta(out.r, out.i)
    ex = excess(G, out, d)
    r = ex.max().item()
    if r > 1.0:
        k = ex.argmax().item()
        raise AssertionError(f"{out.name}: {int((ex > 1).sum())} of {ex.numel()} elements leave the budget, worst {r:.3g} x delta "
                             f"{d:.3g} at element {k}: G {G.view(-1)[k].item()!r} r {out.r.view(-1)[k].item()!r}")
    return r


def cap_holds(out):
    """(c) delta <= 1e-4 max(1, |r|max)."""
    return out.kind == "copy" or delta(out.r, out.i) <= CAP * max(1.0, out.r.abs().max().item())


# ---- the closed forms of the ops, in either precision --------------------------------------------------------------------------

def _view(c, snap, r, n):
    """n floats behind the operand reference r (snap: the arena as the runner left it before the op)."""
    if r.space == rt.SP_NONE:
        return None
    buf, off = {W: (c.weights, r.off), A: (snap, r.off * c.B), S: (c.shr, r.off)}[r.space]
    assert off + n <= buf.numel()
    return buf[off: off + n]


def _wide16(fl):
    return fl.view(BF16).float()


def _silu(x):
    return x / (1.0 + torch.exp(-x))


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))


def _ln(a, eps):
    mean = a.mean(-1, keepdim=True)
    var = ((a - mean) ** 2).mean(-1, keepdim=True)
    return (a - mean) / torch.sqrt(var + eps)


def _prologue(c, snap, op, a, dt):
    """The A-operand prologue of MDT_OP_GEMM / MDT_OP_PREP16 on a [B, R, cin] in precision dt."""
    i, eps = op.i, float(op.f[0])
    cin, pro, B = i[rt.G_CIN], i[rt.G_PRO], a.shape[0]
    if pro == rt.PRO_LAYERNORM:
        return _ln(a, eps) * _view(c, snap, op.p0, cin).to(dt) + _view(c, snap, op.p1, cin).to(dt)
    if pro == rt.PRO_GROUPNORM:
        G, gs = i[rt.G_GROUPS], i[rt.G_GSIZE]
        st = _view(c, snap, op.p2, B * G * 2).view(B, G, 2).to(dt)       # MDT_OP_GN_STATS wrote them: the op's own operand
        grp = torch.clamp(torch.arange(cin) // gs, max=G - 1)
        a = (a - st[:, grp, 0].unsqueeze(1)) * st[:, grp, 1].unsqueeze(1) * _view(c, snap, op.p0, cin).to(dt) + _view(c, snap, op.p1, cin).to(dt)
        if op.p3.space != rt.SP_NONE:
            ss = _view(c, snap, op.p3, 2 * cin).to(dt)
            a = a * (ss[:cin] + 1.0) + ss[cin:]
        return _silu(a) if i[rt.G_PRO_SILU] else a
    if pro == rt.PRO_SILU:
        return _silu(a)
    return a


def _idx(base, rows, ld, col, n):
    """Element indices of columns [col, col + n) of `rows` rows of pitch ld that start at element `base`."""
    return (base + torch.arange(rows).view(-1, 1) * ld + col + torch.arange(n).view(1, -1)).reshape(-1)


def _a_rows(c, snap, op, in16):
    i, B = op.i, c.B
    r_in, lda, cin, col = i[rt.G_R_IN], i[rt.G_LDA], i[rt.G_CIN], i[rt.G_A_COL]
    fl = _view(c, snap, op.a, B * r_in * lda // (2 if in16 else 1))
    return (_wide16(fl) if in16 else fl).view(B, r_in, lda)[:, :, col: col + cin]


def _prep16(c, snap, op, name):
    i, B = op.i, c.B
    r_in, cin = i[rt.G_R_IN], i[rt.G_CIN]
    a = _a_rows(c, snap, op, i[rt.G_WFMT] == 2)
    idx = _idx(2 * op.out.off * B, B * r_in, cin, 0, cin)
    if i[rt.G_PRO] == rt.PRO_NONE:
        return [Out(name, "copy", idx, None, None, rne_bits(a).view(-1))]
    r, ii = (_prologue(c, snap, op, a.to(dt), dt).reshape(-1) for dt in (F64, F32))
    return [Out(name, "bf16", idx, r, ii, None)]


def _gemm(c, snap, op, name):
    i, B = op.i, c.B
    wf = i[rt.G_WFMT]
    r_out, r_in, cin, taps, n, ldc, ocol = i[rt.G_R_OUT], i[rt.G_R_IN], i[rt.G_CIN], i[rt.G_TAPS], i[rt.G_N], i[rt.G_LDC], i[rt.G_O_COL]
    assert wf in (1, 2, 6, 10, 38, 134) and i[rt.G_T_STRIDE] == 1 and i[rt.G_O_STRIDE] == 1 and not i[rt.G_O_OFF] and r_out == r_in == i[rt.G_O_ROWS]
    a32 = _a_rows(c, snap, op, wf != 1)
    w32 = _wide16(_view(c, snap, op.w, n * taps * cin // 2)).view(n, taps, cin)
    bias = _view(c, snap, op.bias, n)
    res = None
    if op.res.space != rt.SP_NONE:
        ldr = i[rt.G_LDR]
        fl = _view(c, snap, op.res, B * r_out * ldr // (2 if wf == 38 else 1))
        res = (_wide16(fl) if wf == 38 else fl).view(B, r_out, ldr)[:, :, :n]
    rows = torch.arange(r_out)

    def form(dt, kernel_fold):
        a = a32.to(dt)
        if wf == 1:                                  # A is consumed as bf16 after the prologue: the mode's one hidden rounding
            a = _prologue(c, snap, op, a, dt).to(BF16).to(dt)
        w = w32.to(dt)

        def product(x):
            acc = torch.zeros(B, r_out, n, dtype=dt)
            for t in range(taps):
                src = rows * 1 + t * i[rt.G_T_DJ] + i[rt.G_T_OFF]
                ok = ((src >= 0) & (src < r_in)).to(dt)
                acc = acc + (x[:, src.clamp(0, r_in - 1), :] * ok.view(1, -1, 1)) @ w[:, t, :].T
            return acc
        if wf == 134 and kernel_fold:                # the kernel's formula: statistics gathered beside the product, applied to the sums
            mean = a.mean(-1, keepdim=True)
            var = ((a * a).mean(-1, keepdim=True) - mean * mean).clamp(min=0.0)
            acc = (1.0 / torch.sqrt(var + float(op.f[0]))) * (product(a) - mean * _view(c, snap, op.p0, n).to(dt))
        elif wf == 134:                              # LayerNorm (its gain folded into W, its bias into `bias`), then the projection
            acc = product(_ln(a, float(op.f[0])))
        else:
            acc = product(a)
        if bias is not None:
            acc = acc + bias.to(dt)
        if i[rt.G_ACT] == 1:
            acc = _gelu(acc)
        if res is not None:
            acc = acc + res.to(dt)
        return acc.reshape(-1)
    r, ii = form(F64, False), form(F32, True)
    if wf in (6, 38, 134):
        return [Out(name, "bf16", _idx(2 * op.out.off * B, B * r_out, ldc, ocol, n), r, ii, None)]
    outs = [Out(name, "f32", _idx(op.out.off * B, B * r_out, ldc, ocol, n), r, ii, None)]
    if wf == 10:                                     # the copy is a rounding of the fp32 output the op itself stored: see outputs()
        outs.append(Out(name + " copy", "copy", _idx(2 * op.p0.off * B, B * r_out, n, 0, n), None, None, None, outs[0].idx))
    return outs


def _gn_act(c, snap, op, name):
    i, B = op.i, c.B
    rows, ld, G, gs = i[rt.N_ROWS], i[rt.N_LD], i[rt.N_GROUPS], i[rt.N_GSIZE]
    eps, s2 = float(op.f[0]), torch.tensor(float(op.f[1]), dtype=F32)
    if op.a2.space != rt.SP_NONE:
        ca = i[rt.N_CA]
        xa, xb = _view(c, snap, op.a, B * rows * ca).view(B, rows, ca), _view(c, snap, op.a2, B * rows * (ld - ca)).view(B, rows, ld - ca)
    else:
        xa, xb = _view(c, snap, op.a, B * rows * ld).view(B, rows, ld), None

    def form(dt):
        x = xa.to(dt) if xb is None else torch.cat([xa.to(dt), xb.to(dt) * s2.to(dt)], dim=2)
        g = x.view(B, rows, G, gs)
        mean = g.mean(dim=(1, 3), keepdim=True)
        var = ((g - mean) ** 2).mean(dim=(1, 3), keepdim=True)
        y = ((g - mean) / torch.sqrt(var + eps)).view(B, rows, ld) * _view(c, snap, op.p0, ld).to(dt) + _view(c, snap, op.p1, ld).to(dt)
        if op.p3.space != rt.SP_NONE:
            ss = _view(c, snap, op.p3, 2 * ld).to(dt)
            y = y * (ss[:ld] + 1.0) + ss[ld:]
        return (_silu(y) if i[rt.N_SILU] else y).reshape(-1)
    r, ii = form(F64), form(F32)
    if i[rt.N_OUT16]:
        outs = [Out(name, "bf16", _idx(2 * op.out.off * B, B * rows, ld, 0, ld), r, ii, None)]
    else:
        outs = [Out(name, "f32", _idx(op.out.off * B, B * rows, ld, 0, ld), r, ii, None)]
    if op.p2.space != rt.SP_NONE:                    # the raw copy: bf16 of the fp32 input, the second source scaled in fp32 first
        src = xa if xb is None else torch.cat([xa, xb * s2], dim=2)
        outs.append(Out(name + " raw copy", "copy", _idx(2 * op.p2.off * B, B * rows, ld, 0, ld), None, None, rne_bits(src).view(-1)))
    return outs


def reference(c, k, before):
    """The output tensors of op k of the case with their references, from the arena as it was before the op."""
    op = c.ops[k]
    name = f"{c.key} op {k}"
    if op.kind == rt.OP_PREP16:
        return _prep16(c, before, op, name)
    if op.kind == rt.OP_GEMM:
        return _gemm(c, before, op, name)
    if op.kind == rt.OP_GN_ACT:
        return _gn_act(c, before, op, name)
    raise ValueError(op.kind)


def outputs(out, after):
    """G of one output tensor in the arena after the op; a MDT_G_WFMT 10 copy gets its expectation here: RNE of the stored fp32."""
    if out.kind == "f32":
        return after[out.idx], out
    G = after.view(BF16)[out.idx]
    if out.src is not None:
        out = out._replace(bits=rne_bits(after[out.src]))
    return G, out


def stepwise(c, runner):
    """Runs the case one op per program; the arena before the first op and after each."""
    snaps = [c.act.clone()]
    for op in c.ops:
        snaps.append(runner([op], c.weights, snaps[-1].clone(), c.shr, c.B))
    return snaps


def verify(c, snaps, judge=check):
    """Every checked op of the case against the criterion; {output name: ratio}.  Whatever is not an output element of an op must
    come back bit for bit -- for the ops that only run (MDT_OP_GN_STATS) that is not looked at."""
    ratios = {}
    for k in c.check:
        before, after = snaps[k], snaps[k + 1]
        mask = torch.zeros(2 * before.numel(), dtype=torch.bool)
        for out in reference(c, k, before):
            G, out = outputs(out, after)
            if out.kind == "f32":
                mask[2 * out.idx] = True
                mask[2 * out.idx + 1] = True
            else:
                mask[out.idx] = True
            ratios[out.name] = judge(G, out)
        b16, a16 = before.view(torch.int16), after.view(torch.int16)
        assert torch.equal(a16[~mask], b16[~mask]), f"{c.key} op {k}: an element that is no output of the op was written"
    return ratios


# ---- inputs --------------------------------------------------------------------------------------------------------------------

def _b16(t):
    return t.to(BF16)


def tie_values():
    """fp32 values a bf16 copy must get exactly right: halfway between two bf16 numbers with the lower neighbour even (rounds
    down) and odd (rounds up), both signs, several binades; just beside the ties; +-0; the largest value whose rounding stays
    finite (0x7f7f7fff) and its negative."""
    pat = []
    for e in (0x3F80, 0x4000, 0x3C00, 0x4780, 0x0080):       # 1, 2, 2^-7, 2^16, the smallest normal binade
        for m in (0, 1, 2, 0x7E, 0x7F):                       # even and odd lower neighbours, the binade's last two
            hi = e + m
            pat += [(hi << 16) | 0x8000, (hi << 16) | 0x7FFF, (hi << 16) | 0x8001]
    pat += [0x00000000, 0x7F7F7FFF]
    pat = torch.tensor(pat + [p | 0x80000000 for p in pat], dtype=torch.int64)
    return (pat - ((pat >> 31) << 32)).to(torch.int32).view(F32)


def plant(x, vals, seed):
    """Scatters vals over the flat fp32 tensor x at fixed pseudo-random places (every value at least once, about 3 % of x)."""
    g = torch.Generator().manual_seed(seed)
    n = max(vals.numel(), x.numel() // 32)
    pos = torch.randperm(x.numel(), generator=g)[:n]
    x[pos] = vals[torch.arange(n) % vals.numel()]
    return x


def near_boundary(p):
    """Prologue values (fp64) within TIE_GUARD of the boundary between two bf16 roundings.  Values below 2^-7 are left alone: the
    guard is a twentieth of their spacing or more, and the other rounding moves an output by at most 2^-15 |w| < 1e-5, inside delta."""
    u = ulp_bf16(p)
    t = p.abs() / u
    return (((t - torch.floor(t) - 0.5).abs() * u) < TIE_GUARD) & (p.abs() >= 2.0 ** -7)


def settle(x, prologue):
    """Moves elements of x (fp32, in place) until no prologue(x) (fp64, same shape) lies near a bf16 rounding boundary."""
    for _ in range(50):
        near = near_boundary(prologue(x.double()))
        if not near.any():
            return x
        x[near] = x[near] * (1 + 3e-5) + 1e-7
    raise AssertionError("settle() did not converge")


def _stats_op(aoff, stoff, R, cin, G):
    st = rt.MdtOp()
    st.kind = rt.OP_GN_STATS
    st.a, st.out = ref(A, aoff), ref(A, stoff)
    st.i[rt.N_ROWS], st.i[rt.N_LD], st.i[rt.N_GROUPS], st.i[rt.N_GSIZE] = R, cin, G, cin // G
    st.f[0] = 1e-5
    return st


def _gn64(x, G, gain, beta, film, silu):
    """GroupNorm prologue in fp64 with the statistics of x itself (for settle())."""
    B, R, cin = x.shape
    g = x.view(B, R, G, cin // G)
    mean = g.mean(dim=(1, 3), keepdim=True)
    var = ((g - mean) ** 2).mean(dim=(1, 3), keepdim=True)
    y = ((g - mean) / torch.sqrt(var + 1e-5)).view(B, R, cin) * gain.double() + beta.double()
    y = y * (film[:cin].double() + 1.0) + film[cin:].double()
    return _silu(y) if silu else y


# ---- cases: k_prep16 -----------------------------------------------------------------------------------------------------------

PREP_SHAPES = [(5, 32, 64), (3, 128, 256), (130, 4, 64)]
PREP_KINDS = ["copy", "ln", "gn", "silu", "ln16"]


def prep16_case(B, R, cin, kind):
    G = 8
    weights = torch.cat([1 + 0.1 * rnd(cin, seed=3), 0.1 * rnd(cin, seed=4)])
    shr = 0.3 * rnd(2 * cin, seed=7)
    in16 = kind == "ln16"
    n_in = R * cin // 2 if in16 else R * cin
    xoff, stoff, ooff = 0, n_in, n_in + 64
    act = torch.zeros(B * (ooff + R * cin // 2))
    x = rnd(B * R * cin, seed=5) * 1.3 + 0.2
    if kind == "copy":
        plant(x, tie_values(), seed=11)
    act[: B * n_in] = pack16(_b16(x)) if in16 else x
    ops = []
    pre = rt.MdtOp()
    pre.kind = rt.OP_PREP16
    pre.a, pre.out = ref(A, xoff), ref(A, ooff)
    pi = pre.i
    pi[rt.G_R_IN], pi[rt.G_LDA], pi[rt.G_CIN] = R, cin, cin
    pre.f[0] = 1e-5
    if kind in ("ln", "ln16"):
        pre.p0, pre.p1, pi[rt.G_PRO] = ref(W, 0), ref(W, cin), rt.PRO_LAYERNORM
        pi[rt.G_WFMT] = 2 if in16 else 0
    elif kind == "gn":
        ops.append(_stats_op(xoff, stoff, R, cin, G))
        pre.p0, pre.p1, pre.p2, pre.p3 = ref(W, 0), ref(W, cin), ref(A, stoff), ref(S, 0)
        pi[rt.G_PRO], pi[rt.G_GROUPS], pi[rt.G_GSIZE], pi[rt.G_PRO_SILU] = rt.PRO_GROUPNORM, G, cin // G, 1
    elif kind == "silu":
        pi[rt.G_PRO] = rt.PRO_SILU
    ops.append(pre)
    return Case(f"prep16 {kind} ({B},{R},{cin})", "k_prep16 " + kind, ops, weights, act, shr, B, [len(ops) - 1], None, None,
                "ties" if kind == "copy" else None)


# ---- cases: MDT_G_WFMT 1 (k_gemm_bf16x3.hip) -----------------------------------------------------------------------------------

WFMT1_CASES = [(3, 16, 128, 96, 3, rt.PRO_GROUPNORM), (5, 64, 32, 64, 3, rt.PRO_NONE), (33, 1, 256, 160, 1, rt.PRO_SILU)]
PRO_NAME = {rt.PRO_NONE: "none", rt.PRO_GROUPNORM: "gn", rt.PRO_SILU: "silu", rt.PRO_LAYERNORM: "ln"}


def wfmt1_case(B, R, cin, N, taps, pro):
    K, G = taps * cin, 8
    hi = pack16(_b16(rnd(N, K, seed=1, scale=K ** -0.5)))
    gain, beta = 1 + 0.1 * rnd(cin, seed=3), 0.1 * rnd(cin, seed=4)
    weights = torch.cat([hi, rnd(N, seed=2), gain, beta])
    o_b, o_g, o_nb = hi.numel(), hi.numel() + N, hi.numel() + N + cin
    xoff, stoff, ooff, roff = 0, R * cin, R * cin + 64, R * cin + 64 + R * N
    shr = 0.3 * rnd(2 * cin, seed=7)
    x = (rnd(B * R * cin, seed=5) * 1.3 + 0.2).view(B, R, cin)
    if pro == rt.PRO_GROUPNORM:
        settle(x, lambda v: _gn64(v, G, gain, beta, shr, True))
    elif pro == rt.PRO_SILU:
        settle(x, _silu)
    act = torch.zeros(B * (roff + R * N))
    act[: B * R * cin] = x.reshape(-1)
    act[B * roff:] = rnd(B * R * N, seed=6)
    ops = [_stats_op(xoff, stoff, R, cin, G)] if pro == rt.PRO_GROUPNORM else []
    op = gemm_op(a=ref(A, xoff), w=ref(W, 0), bias=ref(W, o_b), out=ref(A, ooff), res=ref(A, roff), r_out=R, r_in=R, lda=cin, cin=cin,
                 taps=taps, t_dj=1 if taps > 1 else 0, t_off=-(taps // 2), n=N, ldc=N, o_rows=R, ldr=N, pro=pro, act=0, eps=1e-5)
    if pro == rt.PRO_GROUPNORM:
        op.p0, op.p1, op.p2, op.p3 = ref(W, o_g), ref(W, o_nb), ref(A, stoff), ref(S, 0)
        op.i[rt.G_GROUPS], op.i[rt.G_GSIZE], op.i[rt.G_PRO_SILU] = G, cin // G, 1
    op.i[rt.G_WFMT] = 1
    ops.append(op)
    return Case(f"wfmt1 {PRO_NAME[pro]} ({B},{R},{cin},{N},{taps})", "k_gemm3 WFMT 1 " + PRO_NAME[pro], ops, weights, act, shr, B,
                [len(ops) - 1], None, None, None)


# ---- cases: k_gemm_b16 ---------------------------------------------------------------------------------------------------------

TILES = [-1, 0, 1, 2]
B16_SHAPES = [(5, 32, 64, 96, 3), (3, 128, 256, 256, 1)]


def b16_case(B, R, cin, N, taps, wf, gelu, tile, w16):
    """One k_gemm_b16 op on a bf16 A: WFMT 2 (fp32 out + fp32 residual), 6 (bf16 out), 10 (fp32 out + residual + bf16 copy; the
    first four output columns have zero weights and bias, and residual rows of tie_values(): the fp32 output IS a tie there)."""
    K = taps * cin
    w = rnd(N, K, seed=1, scale=K ** -0.5)
    bias = rnd(N, seed=2)
    res = rnd(B * R * N, seed=6).view(B * R, N)
    if wf == 10:
        w[:4], bias[:4] = 0.0, 0.0
        t = tie_values()
        t = t[t.abs() < 4.0]                  # (the fp32 output is checked against delta as well: its scale stays the GEMM's)
        res[:, :4] = t[torch.arange(B * R * 4) % t.numel()].view(B * R, 4)
    hi = pack16(_b16(w))
    weights = torch.cat([hi, bias])
    # per-sample arena (floats): [a16 (R cin / 2) | out (R N, or R N / 2 as bf16) | res (R N) | copy16 (R N / 2)]
    aoff, ooff = 0, R * cin // 2
    roff = ooff + (R * N // 2 if wf == 6 else R * N)
    coff = roff + R * N
    act = torch.zeros(B * (coff + R * N // 2))
    act[: B * ooff] = pack16(_b16(rnd(B * R * cin, seed=5) * 1.3 + 0.2))
    act[B * roff: B * coff] = res.reshape(-1)
    op = gemm_op(a=ref(A, aoff), w=ref(W, 0), bias=ref(W, hi.numel()), out=ref(A, ooff), r_out=R, r_in=R, lda=cin, cin=cin, taps=taps,
                 t_dj=1 if taps > 1 else 0, t_off=-(taps // 2), n=N, ldc=N, o_rows=R, act=int(gelu))
    if wf != 6:
        op.res = ref(A, roff)
        op.i[rt.G_LDR] = N
    if wf == 10:
        op.p0 = ref(A, coff)
    op.i[rt.G_WFMT] = wf
    return Case(f"b16 wfmt{wf}{' gelu' if gelu else ''} ({B},{R},{cin},{N},{taps}) tile {tile} w16 {w16}", f"k_gemm_b16 WFMT {wf}",
                [op], weights, act, torch.zeros(4), B, [0], tile, w16, "ties" if wf == 10 else None)


def single_chunk_case(tile, w16):
    """(83, 4, 64, 64): K = 64 is ONE chunk, the residual is requested before the loop; WFMT 38 in place on the stream."""
    B, R, C = 83, 4, 64
    w = pack16(_b16(rnd(C, C, seed=1, scale=C ** -0.5)))
    weights = torch.cat([w, rnd(C, seed=2)])
    act = torch.zeros(B * R * C)
    act[: B * R * C // 2] = pack16(_b16(rnd(B * R * C, seed=3) * 1.5 + 0.3))
    act[B * R * C // 2:] = pack16(_b16(rnd(B * R * C, seed=4)))
    g = gemm_op(a=ref(A, R * C // 2), w=ref(W, 0), bias=ref(W, w.numel()), out=ref(A, 0), res=ref(A, 0), r_out=R, r_in=R, lda=C, cin=C,
                taps=1, n=C, ldc=C, o_rows=R, ldr=C)
    g.i[rt.G_WFMT] = 38
    return Case(f"b16 wfmt38 one chunk (83,4,64,64) tile {tile} w16 {w16}", "k_gemm_b16 WFMT 38", [g], weights, act, torch.zeros(4), B,
                [0], tile, w16, None)


CHAIN_SHAPES = [(130, 4, 64), (5, 32, 512)]


def chain_case(B, R, C, tile, w16):
    """The residual-stream chain of a transformer block: PREP16 (WFMT 2: LayerNorm of the bf16 stream) -> WFMT 6 (GELU, bf16
    hidden) -> WFMT 38 (bf16 residual, in place on the stream); C -> 2 C -> C.  Every op is checked on the bits it read."""
    Hd = 2 * C
    w1, w2 = pack16(_b16(rnd(Hd, C, seed=1, scale=C ** -0.5))), pack16(_b16(rnd(C, Hd, seed=2, scale=Hd ** -0.5)))
    weights = torch.cat([w1, w2, rnd(Hd, seed=3), rnd(C, seed=4), 1 + 0.1 * rnd(C, seed=6), 0.1 * rnd(C, seed=7)])
    o_w2 = w1.numel()
    o_b1 = o_w2 + w2.numel()
    o_b2, o_g, o_be = o_b1 + Hd, o_b1 + Hd + C, o_b1 + Hd + 2 * C
    xoff, lnoff, hoff = 0, R * C // 2, R * C
    act = torch.zeros(B * (hoff + R * Hd // 2))
    act[: B * R * C // 2] = pack16(_b16(rnd(B * R * C, seed=5) * 1.5 + 0.3))
    pre = rt.MdtOp()
    pre.kind = rt.OP_PREP16
    pre.a, pre.out, pre.p0, pre.p1 = ref(A, xoff), ref(A, lnoff), ref(W, o_g), ref(W, o_be)
    pre.i[rt.G_R_IN], pre.i[rt.G_LDA], pre.i[rt.G_CIN], pre.i[rt.G_PRO], pre.i[rt.G_WFMT] = R, C, C, rt.PRO_LAYERNORM, 2
    pre.f[0] = 1e-5
    g1 = gemm_op(a=ref(A, lnoff), w=ref(W, 0), bias=ref(W, o_b1), out=ref(A, hoff), r_out=R, r_in=R, lda=C, cin=C, taps=1, n=Hd, ldc=Hd,
                 o_rows=R, act=1)
    g1.i[rt.G_WFMT] = 6
    g2 = gemm_op(a=ref(A, hoff), w=ref(W, o_w2), bias=ref(W, o_b2), out=ref(A, xoff), res=ref(A, xoff), r_out=R, r_in=R, lda=Hd, cin=Hd,
                 taps=1, n=C, ldc=C, o_rows=R, ldr=C)
    g2.i[rt.G_WFMT] = 38
    return Case(f"b16 chain ({B},{R},{C}) tile {tile} w16 {w16}", "k_gemm_b16 chain (PREP16 WFMT 2, WFMT 6 GELU, WFMT 38)", [pre, g1, g2],
                weights, act, torch.zeros(4), B, [0, 1, 2], tile, w16, None)


FOLD_SHAPES = [(67, 2, 64, 128), (130, 4, 256, 768)]
FOLD_FAMILIES = {"mean 0.7": (0.7, 1.5), "mean 4": (4.0, 0.5)}      # (mean, std) of the rows: "the cancellation case", and a harder one


def column_block_case(fold, family, tile, w16):
    """(41, 8, 256, 128) written as bf16 into columns [64, 192) of rows of 320 (GELU): WFMT 6, or 134 with the LayerNorm folded."""
    return _fold_or_block(41, 8, 256, 128, 320, 64, fold, family, 1, tile, w16)


def fold_case(B, R, C, N, family, tile):
    return _fold_or_block(B, R, C, N, N, 0, True, family, 0, tile, None)


def _fold_or_block(B, R, C, N, LDC, OCOL, fold, family, gelu, tile, w16):
    mean, std = FOLD_FAMILIES[family]
    gam, bet = 1 + 0.2 * rnd(C, seed=2), 0.2 * rnd(C, seed=3)
    wq = rnd(N, C, seed=4, scale=C ** -0.5)
    w2 = _b16((wq * gam.unsqueeze(0)) if fold else wq)
    csum = w2.float().sum(dim=1)
    bias = (wq @ bet if fold else torch.zeros(N)) + 0.1 * rnd(N, seed=5)
    weights = torch.cat([pack16(w2), csum, bias])
    o_cs = w2.numel() // 2
    ooff = R * C // 2
    act = torch.zeros(B * (ooff + R * LDC // 2))
    act[: B * ooff] = pack16(_b16(rnd(B * R * C, seed=7) * std + mean))
    act[B * ooff:] = pack16(_b16(torch.full((B * R * LDC,), 3.0)))
    g = gemm_op(a=ref(A, 0), w=ref(W, 0), bias=ref(W, o_cs + N), out=ref(A, ooff), r_out=R, r_in=R, lda=C, cin=C, taps=1, n=N, ldc=LDC,
                o_rows=R, o_col=OCOL, act=gelu)
    g.i[rt.G_WFMT] = 6
    if fold:
        g.p0 = ref(W, o_cs)
        g.i[rt.G_WFMT] = 134
        g.f[0] = 1e-5
    block = f" into ({LDC}, {OCOL})" if LDC != N else ""
    key = f"b16 wfmt{134 if fold else 6}{block} ({B},{R},{C},{N}){' ' + family if fold else ''} tile {tile}" + (f" w16 {w16}" if w16 is not None else "")
    site = ("k_gemm_b16 WFMT 134 " + family) if fold else "k_gemm_b16 WFMT 6"
    return Case(key, site + (" column block" if block else ""), [g], weights, act, torch.zeros(4), B, [0], tile, w16, None)


# ---- cases: k_norm.hip ---------------------------------------------------------------------------------------------------------

# one shape per dispatch branch of launch_gn_act (the table of tests/test_gpu_poison.py), here with the bf16 store: (B, R, C, G, film, silu)
GN_ACT_SHAPES = [(2, 4, 256, 32, False, False), (3, 16, 128, 8, True, True), (5, 64, 64, 1, False, True), (2, 64, 128, 1, False, True),
                 (2, 16, 512, 8, True, True), (3, 32, 512, 8, True, True), (2, 32, 1024, 8, False, True), (2, 128, 256, 4, False, True),
                 (3, 32, 512, 32, False, False), (2, 48, 512, 32, True, True)]
GN_TWO_SHAPES = [(3, 4, 64, 4, 0.7071), (37, 8, 1024, 8, 0.5)]


def gn_act_case(B, R, C, G, film, silu):
    weights = torch.cat([1 + 0.1 * rnd(C, seed=2), 0.1 * rnd(C, seed=3)])
    shr = 0.3 * rnd(2 * C, seed=9)
    act = torch.cat([rnd(B * R * C, seed=4) * 1.5 + 0.3, torch.zeros(B * R * C // 2)])
    op = rt.MdtOp()
    op.kind = rt.OP_GN_ACT
    op.a, op.out, op.p0, op.p1 = ref(A, 0), ref(A, R * C), ref(W, 0), ref(W, C)
    if film:
        op.p3 = ref(S, 0)
    op.i[rt.N_ROWS], op.i[rt.N_LD], op.i[rt.N_GROUPS], op.i[rt.N_GSIZE], op.i[rt.N_SILU], op.i[rt.N_OUT16] = R, C, G, C // G, int(silu), 1
    op.f[0] = 1e-5
    return Case(f"gn_act ({B},{R},{C},{G}){' film' if film else ''}{' silu' if silu else ''}", "k_gn_act bf16 output", [op], weights, act,
                shr, B, [0], None, None, None)


def gn_two_case(B, R, C, G, scale2):
    """cat([a, SCALE2 a2]) from its two sources: bf16 normalised + SiLU output and the raw bf16 copy.  The copy's sources hold the
    ties (no value beyond 2^17: the statistics must stay finite); SCALE2 = 0.5 keeps a tie of a2 a tie of the product."""
    ld = 2 * C
    weights = torch.cat([1 + 0.1 * rnd(ld, seed=2), 0.1 * rnd(ld, seed=3)])
    aoff, boff, yoff = 0, R * C, 2 * R * C
    roff = yoff + R * ld // 2
    act = torch.zeros(B * (roff + R * ld // 2))
    t = tie_values()
    t = t[t.abs() < 4.0]                  # ties of the binades 2^-126, 2^-7, 1 and 2: the group statistics keep their scale
    xa, xb = plant(rnd(B * R * C, seed=4) * 1.5 + 0.3, t, seed=12), plant(rnd(B * R * C, seed=5) * 0.8 - 0.2, t, seed=13)
    act[: B * R * C], act[B * boff: B * yoff] = xa, xb
    op = rt.MdtOp()
    op.kind = rt.OP_GN_ACT
    op.a, op.a2, op.out, op.p0, op.p1, op.p2 = ref(A, aoff), ref(A, boff), ref(A, yoff), ref(W, 0), ref(W, ld), ref(A, roff)
    i = op.i
    i[rt.N_ROWS], i[rt.N_LD], i[rt.N_GROUPS], i[rt.N_GSIZE], i[rt.N_SILU], i[rt.N_OUT16], i[rt.N_CA] = R, ld, G, ld // G, 1, 1, C
    op.f[0], op.f[1] = 1e-5, scale2
    return Case(f"gn_act two sources ({B},{R},{C},{G}) scale2 {scale2}", "k_gn_act two sources + raw copy", [op], weights, act,
                torch.zeros(4), B, [0], None, None, "ties")


# ---- the list ------------------------------------------------------------------------------------------------------------------

def all_cases():
    """(key, builder) of every case of the GPU file, in its order; builders are called lazily (and cached by the test files)."""
    cs = []

    def add(fn, *args):
        cs.append((fn, args))
    for shape in PREP_SHAPES:
        for kind in PREP_KINDS:
            add(prep16_case, *shape, kind)
    for case in WFMT1_CASES:
        add(wfmt1_case, *case)
    for tile in TILES:
        for shape in B16_SHAPES:
            add(b16_case, *shape, 2, 0, tile, None)
            add(b16_case, *shape, 10, 0, tile, None)
            for w16 in (1, 0):
                for gelu in (0, 1):
                    add(b16_case, *shape, 6, gelu, tile, w16)
        for w16 in (1, 0):
            add(single_chunk_case, tile, w16)
            for shape in CHAIN_SHAPES:
                add(chain_case, *shape, tile, w16)
            add(column_block_case, False, "mean 0.7", tile, w16)
        for family in FOLD_FAMILIES:
            for shape in FOLD_SHAPES:
                add(fold_case, *shape, family, tile)
            add(column_block_case, True, family, tile, None)
    for shape in GN_ACT_SHAPES:
        add(gn_act_case, *shape)
    for shape in GN_TWO_SHAPES:
        add(gn_two_case, *shape)
    return cs


_BUILT = {}


def build(fn, args):
    k = (fn.__name__,) + tuple(args)
    if k not in _BUILT:
        _BUILT[k] = fn(*args)
    return _BUILT[k]


def case_id(fn, args):
    return fn.__name__[:-5] + "-" + "-".join(str(a).replace(" ", "") for a in args)
