"""The programs of tests/test_gpu_ops.py as functions (no GPU in here): one op, or one op chain, with its seeded weights and the
arena it runs on.  tests/test_gpu_ops.py runs them on the inputs they have always had (the defaults below); tests/norm_ref.py
hands the same programs other inputs (`x=`), another eps, fp32 instead of bf16 output.  Every builder returns a namespace with
ops, weights, act, shr, B, the named parameter tensors the closed forms need, and the arena offsets of its tensors."""
from types import SimpleNamespace as NS

import torch

from moleculediffusiontransformer_amd import runtime as rt

W, A, S = rt.SP_WEIGHT, rt.SP_ACT, rt.SP_SHR


def ref(space, off=0):
    return rt.MdtRef(space, 0, off)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _flat(x, default):
    return default if x is None else x.reshape(-1).contiguous().float()


def gemm_op(**kw):
    op = rt.MdtOp()
    op.kind = rt.OP_GEMM
    for k in ("a", "w", "bias", "out", "res", "p0", "p1", "p2", "p3"):
        if k in kw:
            setattr(op, k, kw.pop(k))
    i = op.i
    i[rt.G_T_STRIDE], i[rt.G_O_STRIDE] = 1, 1
    names = dict(r_out=rt.G_R_OUT, r_in=rt.G_R_IN, lda=rt.G_LDA, cin=rt.G_CIN, taps=rt.G_TAPS, t_stride=rt.G_T_STRIDE,
                 t_dj=rt.G_T_DJ, t_off=rt.G_T_OFF, n=rt.G_N, ldc=rt.G_LDC, o_rows=rt.G_O_ROWS,
                 o_stride=rt.G_O_STRIDE, o_off=rt.G_O_OFF, ldr=rt.G_LDR, pro=rt.G_PRO, groups=rt.G_GROUPS,
                 gsize=rt.G_GSIZE, pro_silu=rt.G_PRO_SILU, act=rt.G_ACT, m_mode=rt.G_M_MODE, a_col=rt.G_A_COL,
                 o_col=rt.G_O_COL)
    op.f[0] = kw.pop("eps", 0.0)
    for k, v in kw.items():
        i[names[k]] = v
    return op


def gn_stats_op(xoff, stoff, rows, ld, groups, gsize, eps):
    """MDT_OP_GN_STATS: (mean, rstd) of every (sample, group), 2 G floats per sample at ACT offset stoff."""
    st = rt.MdtOp()
    st.kind = rt.OP_GN_STATS
    st.a, st.out = ref(A, xoff), ref(A, stoff)
    st.i[rt.N_ROWS], st.i[rt.N_LD], st.i[rt.N_GROUPS], st.i[rt.N_GSIZE] = rows, ld, groups, gsize
    st.f[0] = eps
    return st


def split_planes(w):
    hi = w.to(torch.bfloat16)
    lo = (w - hi.float()).to(torch.bfloat16)
    return hi.contiguous().view(-1).view(torch.float32), lo.contiguous().view(-1).view(torch.float32)


def layernorm_gemm(B, R, C, N, x=None, eps=1e-5):
    """k_gemm with the LayerNorm prologue (test_gemm_layernorm_prologue).  Arena: [x (B R C) | out (B R N)]."""
    w, g, b = rnd(N, C, seed=1, scale=C ** -0.5), 1 + 0.1 * rnd(C, seed=2), 0.1 * rnd(C, seed=3)
    weights = torch.cat([w.view(-1), g, b])
    act = torch.cat([_flat(x, rnd(B * R * C, seed=4) * 2 + 0.5), torch.zeros(B * R * N)])
    ops = [gemm_op(a=ref(A, 0), w=ref(W, 0), out=ref(A, R * C), p0=ref(W, N * C), p1=ref(W, N * C + C), r_out=R,
                   r_in=R, lda=C, cin=C, taps=1, n=N, ldc=N, o_rows=R, pro=rt.PRO_LAYERNORM, eps=eps)]
    return NS(ops=ops, weights=weights, act=act, shr=torch.zeros(4), B=B, w=w, g=g, b=b)


def groupnorm_gemm(B, R, C, G, N, film, silu, eps, x=None):
    """MDT_OP_GN_STATS, then k_gemm with the GroupNorm (+ FiLM + SiLU) prologue (test_gn_stats_and_groupnorm_prologue); three
    taps where there is a SiLU.  Per-sample arena: [x (R C) | stats (64) | out (R N)] -- the statistics are 2 G <= 64 floats."""
    gs = C // G
    taps = 3 if silu else 1
    K = taps * C
    w, g, b = rnd(N, K, seed=1, scale=K ** -0.5), 1 + 0.1 * rnd(C, seed=2), 0.1 * rnd(C, seed=3)
    weights = torch.cat([w.view(-1), g, b])
    shr = 0.3 * rnd(2 * C, seed=9)
    xoff, stoff, ooff = 0, R * C, R * C + 64
    act = torch.zeros(B * (R * C + 64 + R * N))
    act[: B * R * C] = _flat(x, rnd(B * R * C, seed=4) * 1.5 + 0.3)
    ops = [gn_stats_op(xoff, stoff, R, C, G, gs, eps),
           gemm_op(a=ref(A, xoff), w=ref(W, 0), out=ref(A, ooff), p0=ref(W, N * K), p1=ref(W, N * K + C),
                   p2=ref(A, stoff), p3=ref(S, 0) if film else ref(rt.SP_NONE), r_out=R, r_in=R, lda=C, cin=C,
                   taps=taps, t_dj=1 if taps > 1 else 0, t_off=-(taps // 2), n=N, ldc=N, o_rows=R,
                   pro=rt.PRO_GROUPNORM, groups=G, gsize=gs, pro_silu=int(silu))]
    return NS(ops=ops, weights=weights, act=act, shr=shr, B=B, w=w, g=g, b=b, taps=taps, K=K, stoff=stoff, ooff=ooff)


def split_gemm(B, R, cin, N, taps, pro, x=None, eps=1e-5):
    """k_gemm3 / k_gemm_as on split-bf16 weight planes (test_gemm_split_bf16): prologue `pro` (GroupNorm with 8 groups, FiLM and
    SiLU after MDT_OP_GN_STATS; LayerNorm; SiLU; none), bias, residual.  Per-sample arena: [x (R cin) | stats (64) | out (R N) |
    residual (R N)]."""
    K = taps * cin
    w = rnd(N, K, seed=1, scale=K ** -0.5)
    hi, lo = split_planes(w)
    G = 8
    gs = cin // G
    bias, g, b = rnd(N, seed=2), 1 + 0.1 * rnd(cin, seed=3), 0.1 * rnd(cin, seed=4)
    weights = torch.cat([hi, lo, bias, g, b])
    o_hi, o_lo, o_b, o_g, o_nb = 0, hi.numel(), 2 * hi.numel(), 2 * hi.numel() + N, 2 * hi.numel() + N + cin
    xoff, stoff, ooff, roff = 0, R * cin, R * cin + 64, R * cin + 64 + R * N
    act = torch.zeros(B * (roff + R * N))
    act[: B * R * cin] = _flat(x, rnd(B * R * cin, seed=5) * 1.3 + 0.2)
    res = rnd(B * R * N, seed=6)
    act[B * roff:] = res
    shr = 0.3 * rnd(2 * cin, seed=7)
    ops = []
    if pro == rt.PRO_GROUPNORM:
        ops.append(gn_stats_op(xoff, stoff, R, cin, G, gs, eps))
    op = gemm_op(a=ref(A, xoff), w=ref(W, o_hi), bias=ref(W, o_b), out=ref(A, ooff), res=ref(A, roff),
                 p0=ref(W, o_g), p1=ref(W, o_nb), p2=ref(A, stoff), p3=ref(S, 0), r_out=R, r_in=R, lda=cin, cin=cin,
                 taps=taps, t_dj=1 if taps > 1 else 0, t_off=-(taps // 2), n=N, ldc=N, o_rows=R, ldr=N, pro=pro,
                 groups=G, gsize=gs, pro_silu=1, act=0, eps=eps)
    op.a2 = ref(W, o_lo)
    ops.append(op)
    return NS(ops=ops, weights=weights, act=act, shr=shr, B=B, w=w, bias=bias, g=g, b=b, res=res, G=G, K=K,
              stoff=stoff, ooff=ooff, roff=roff)


def gn_act(B, R, C, G, film, silu, eps, x=None):
    """k_gn_act, one source, fp32 output (test_gn_act).  Arena: [x (B R C) | y (B R C)]."""
    g, b = 1 + 0.1 * rnd(C, seed=2), 0.1 * rnd(C, seed=3)
    weights = torch.cat([g, b])
    shr = 0.3 * rnd(2 * C, seed=9)
    act = torch.cat([_flat(x, rnd(B * R * C, seed=4) * 1.5 + 0.3), torch.zeros(B * R * C)])
    op = rt.MdtOp()
    op.kind = rt.OP_GN_ACT
    op.a, op.out, op.p0, op.p1 = ref(A, 0), ref(A, R * C), ref(W, 0), ref(W, C)
    if film:
        op.p3 = ref(S, 0)
    op.i[rt.N_ROWS], op.i[rt.N_LD], op.i[rt.N_GROUPS], op.i[rt.N_GSIZE], op.i[rt.N_SILU] = R, C, G, C // G, int(silu)
    op.f[0] = eps
    return NS(ops=[op], weights=weights, act=act, shr=shr, B=B, g=g, b=b)


def gn_act_two_sources(B, R, C, G, scale2=0.7071, out16=True, xa=None, xb=None, eps=1e-5):
    """k_gn_act on cat([a, scale2 * a2]) read from its two sources, SiLU (test_gn_act_on_two_sources_with_raw_copy).  out16: the
    output is bf16 and a raw bf16 copy of the input goes to p2; otherwise fp32 output, no copy.  Per-sample arena (floats):
    [a (R C) | a2 (R C) | y (R ld / 2, or R ld) | raw16 (R ld / 2, or nothing)]."""
    ld = 2 * C
    g, b = 1 + 0.1 * rnd(ld, seed=2), 0.1 * rnd(ld, seed=3)
    weights = torch.cat([g, b])
    aoff, boff, yoff = 0, R * C, 2 * R * C
    roff = yoff + (R * ld // 2 if out16 else R * ld)
    act = torch.zeros(B * (roff + (R * ld // 2 if out16 else 0)))
    xa, xb = _flat(xa, rnd(B * R * C, seed=4) * 1.5 + 0.3), _flat(xb, rnd(B * R * C, seed=5) * 0.8 - 0.2)
    act[: B * R * C], act[B * boff: B * yoff] = xa, xb
    op = rt.MdtOp()
    op.kind = rt.OP_GN_ACT
    op.a, op.a2, op.out, op.p0, op.p1 = ref(A, aoff), ref(A, boff), ref(A, yoff), ref(W, 0), ref(W, ld)
    if out16:
        op.p2 = ref(A, roff)
    i = op.i
    i[rt.N_ROWS], i[rt.N_LD], i[rt.N_GROUPS], i[rt.N_GSIZE], i[rt.N_SILU], i[rt.N_OUT16], i[rt.N_CA] = R, ld, G, ld // G, 1, int(out16), C
    op.f[0], op.f[1] = eps, scale2
    return NS(ops=[op], weights=weights, act=act, shr=torch.zeros(4), B=B, g=g, b=b, xa=xa, xb=xb, ld=ld, yoff=yoff, roff=roff)


def ring_projection(B, R, cin, N, ln, res, prod, x=None, eps=1e-5):
    """k_proj (MDT_G_WFMT 16 / 17, test_row_stationary_projection_on_ring_tiles): LayerNorm prologue without affine ("plain"), with
    gain / bias vectors ("affine") or none, bias, residual in place on the output.  Arena: [x (B R cin) | out (B R N)]."""
    from moleculediffusiontransformer_amd.compiler import UNetCompiler
    w = rnd(N, cin, seed=1, scale=cin ** -0.5)
    f32 = prod == "f32"                  # MDT_G_WFMT = 17: fp32 fragment tiles, exact fp32 MFMA products
    tile = UNetCompiler._tile_f32 if f32 else UNetCompiler._tile
    tiles = [tile(w[64 * c: 64 * c + 64, 128 * h: 128 * h + 128]) for c in range(N // 64) for h in range(cin // 128)]
    wt = torch.cat(tiles)
    bias, g, b = rnd(N, seed=2), 1 + 0.1 * rnd(cin, seed=5), 0.1 * rnd(cin, seed=6)
    weights = torch.cat([wt, bias, g, b])
    nb = wt.numel()
    x = _flat(x, rnd(B * R * cin, seed=3) * 1.3 + 0.2)
    out0 = rnd(B * R * N, seed=4)
    act = torch.cat([x, out0])
    op = gemm_op(a=ref(A, 0), w=ref(W, 0), bias=ref(W, nb), out=ref(A, R * cin), r_out=R, r_in=R, lda=cin, cin=cin, taps=1, n=N,
                 ldc=N, o_rows=R, eps=eps)
    if ln:
        op.i[rt.G_PRO] = rt.PRO_LAYERNORM
        if ln == "affine":
            op.p0, op.p1 = ref(W, nb + N), ref(W, nb + N + cin)
    if res:
        op.res = ref(A, R * cin)
        op.i[rt.G_LDR] = N
    op.i[rt.G_WFMT] = 17 if f32 else 16
    return NS(ops=[op], weights=weights, act=act, shr=torch.zeros(4), B=B, w=w, bias=bias, g=g, b=b, x=x, out0=out0, nb=nb)


def _rconv_compiler(prod):
    from moleculediffusiontransformer_amd.compiler import UNetCompiler
    from moleculediffusiontransformer_amd.netspec import inverse_unet_config
    return UNetCompiler(inverse_unet_config(16, 64, 128, 12), 64, 12, {}, gemm_mode=prod)


def ring_conv(C, T, B, taps, gsize, film, silu, res, in_scale, prod, x=None, eps=None):
    """k_rconv (test_row_stationary_conv): GroupNorm + FiLM + SiLU prologue, k = 1 | 3 convolution, residual from another tensor
    ("other") or accumulated in place ("accumulate").  Arena: [x | out | other], B T C floats each.  eps: 1e-6 for a k = 1
    convolution (Transformer1d.to_in), 1e-5 otherwise, unless given."""
    from moleculediffusiontransformer_amd.compiler import Ten
    comp = _rconv_compiler(prod)
    w = rnd(C, C, taps, seed=1, scale=(C * taps) ** -0.5)
    gb = torch.cat([1 + 0.1 * rnd(C, seed=2), 0.1 * rnd(C, seed=3), 0.1 * rnd(C, seed=5)])   # gain | beta | conv bias
    g_off = comp.W.add("gb", gb)
    xt, out, other = Ten(A, 0, T, C), Ten(A, T * C, T, C), Ten(A, 2 * T * C, T, C)
    if eps is None:
        eps = 1e-6 if taps == 1 else 1e-5
    comp.rconv(xt, w, "w", out, taps=taps, bias_off=None if res == "accumulate" else g_off + 2 * C,
               res={"other": other, "accumulate": out, None: None}[res],
               gn=(g_off, g_off + C, gsize, eps, silu) if gsize else None, in_scale=in_scale)
    op = comp.ops[0]
    if film:
        op.p3 = ref(S, 0)
    shr = 0.3 * rnd(2 * C, seed=9)
    act = torch.cat([_flat(x, rnd(B * T * C, seed=4) * 1.5 + 0.3), rnd(B * T * C, seed=6), rnd(B * T * C, seed=7)])
    return NS(ops=[op], weights=comp.W.pack(), act=act, shr=shr, B=B, w=w, gb=gb, eps=eps)


def ring_conv_two_sources(C, T, B, taps, gsize, silu, in_scale2, prod, xa=None, xb=None, eps=1e-5):
    """k_rconv on cat([xa, in_scale2 * xb]) that is never materialised (test_row_stationary_conv_two_sources).
    Arena: [xa | out | xb], B T C floats each."""
    from moleculediffusiontransformer_amd.compiler import Ten
    comp = _rconv_compiler(prod)
    w = rnd(C, 2 * C, taps, seed=1, scale=(2 * C * taps) ** -0.5)
    gb = torch.cat([1 + 0.1 * rnd(2 * C, seed=2), 0.1 * rnd(2 * C, seed=3), 0.1 * rnd(C, seed=5)])   # gain | beta | conv bias
    g_off = comp.W.add("gb", gb)
    ta, out, tb = Ten(A, 0, T, C), Ten(A, T * C, T, C), Ten(A, 2 * T * C, T, C)
    comp.rconv(ta, w, "w", out, taps=taps, bias_off=g_off + 4 * C,
               gn=(g_off, g_off + 2 * C, gsize, eps, silu) if gsize else None, x2=tb, in_scale2=in_scale2)
    act = torch.cat([_flat(xa, rnd(B * T * C, seed=4) * 1.5 + 0.3), rnd(B * T * C, seed=6), _flat(xb, rnd(B * T * C, seed=7) * 0.8 - 0.2)])
    return NS(ops=[comp.ops[0]], weights=comp.W.pack(), act=act, shr=torch.zeros(4), B=B, w=w, gb=gb)


def resblock_case(cin, cout, film, prod="bf16x3", scale1=1.0, shift1=0.0):
    """One MDT_OP_RESBLOCK op with seeded weights + the closed form of the reference block (modules.py:145-205).  scale1 multiplies
    the first convolution's weight and bias (the second GroupNorm then sees values of that scale), shift1 is added to its bias."""
    from moleculediffusiontransformer_amd.compiler import Ten, UNetCompiler
    from moleculediffusiontransformer_amd.netspec import inverse_unet_config
    p = "blk."
    sd = {p + "block1.groupnorm.weight": 1 + 0.1 * rnd(cin, seed=1), p + "block1.groupnorm.bias": 0.1 * rnd(cin, seed=2),
          p + "block1.project.weight": rnd(cout, cin, 3, seed=3, scale=(3 * cin) ** -0.5) * scale1,
          p + "block1.project.bias": 0.1 * rnd(cout, seed=4) * scale1 + shift1,
          p + "block2.groupnorm.weight": 1 + 0.1 * rnd(cout, seed=5), p + "block2.groupnorm.bias": 0.1 * rnd(cout, seed=6),
          p + "block2.project.weight": rnd(cout, cout, 3, seed=7, scale=(3 * cout) ** -0.5),
          p + "block2.project.bias": 0.1 * rnd(cout, seed=8),
          p + "to_out.weight": rnd(cout, cin, 1, seed=9, scale=cin ** -0.5), p + "to_out.bias": 0.1 * rnd(cout, seed=10)}
    comp = UNetCompiler(inverse_unet_config(16, 64, 128, 12), 64, 12, sd, gemm_mode=prod)
    cin_p, cout_p = (cin + 15) // 16 * 16, (cout + 15) // 16 * 16        # the op works on channel counts padded to 16
    x = Ten(A, 0, 64, cin_p, cin)
    assert comp.resblock_ok(64, cin, cout, 1, p)
    comp.resnet(x, p, cin, cout, 1, free_input=False)
    assert len(comp.ops) == 1 and comp.ops[0].kind == rt.OP_RESBLOCK
    op = comp.ops[0]
    op.out = ref(A, 64 * cin_p)
    op.p3 = ref(S, 0) if film else ref(0, 0)
    shr = torch.zeros(2 * cout_p)                      # [scale(cout_p) | shift(cout_p)], zero on the padding
    shr[:cout], shr[cout_p: cout_p + cout] = 0.3 * rnd(cout, seed=11), 0.3 * rnd(cout, seed=12)

    def closed_form(xin):                              # xin [B, 64, cin]
        F = torch.nn.functional
        xt = xin.transpose(1, 2)
        h = F.conv1d(F.silu(F.group_norm(xt, 1, sd[p + "block1.groupnorm.weight"], sd[p + "block1.groupnorm.bias"], 1e-5)),
                     sd[p + "block1.project.weight"], sd[p + "block1.project.bias"], padding=1)
        h = F.group_norm(h, 1, sd[p + "block2.groupnorm.weight"], sd[p + "block2.groupnorm.bias"], 1e-5)
        if film:
            h = h * (shr[:cout].view(1, cout, 1) + 1) + shr[cout_p: cout_p + cout].view(1, cout, 1)
        yt = F.conv1d(F.silu(h), sd[p + "block2.project.weight"], sd[p + "block2.project.bias"], padding=1)
        return (yt + F.conv1d(xt, sd[p + "to_out.weight"], sd[p + "to_out.bias"])).transpose(1, 2)
    return comp, op, shr, closed_form, sd


def transformer_sd(p, C, layers, cross, ctx=128, mid=512, seed0=100):
    """Random Transformer1d parameters with the reference's key names (modules.py:469-524)."""
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


def handoff_ext(B, T):
    """bindings.ext[3] / [4] of a pair-split MDT_OP_TF256 / MDT_OP_RES256: zeroed flag words, hand-off blocks (engine.py sizes
    them alike)."""
    nrb = (B * T + 31) // 32
    return {3: torch.zeros(64 + 64 * nrb), 4: torch.zeros(2 * nrb * 2 * 32 * 256)}


def resnet_sd(p, c, cin, seed0):
    r = lambda *sh, seed, scale=1.0: rnd(*sh, seed=seed0 + seed, scale=scale)   # noqa: E731
    sd = {p + "block1.groupnorm.weight": 1 + 0.2 * r(cin, seed=1), p + "block1.groupnorm.bias": 0.2 * r(cin, seed=2),
          p + "block1.project.weight": r(c, cin, 3, seed=3, scale=(3 * cin) ** -0.5), p + "block1.project.bias": 0.1 * r(c, seed=4),
          p + "block2.groupnorm.weight": 1 + 0.2 * r(c, seed=5), p + "block2.groupnorm.bias": 0.2 * r(c, seed=6),
          p + "block2.project.weight": r(c, c, 3, seed=7, scale=(3 * c) ** -0.5), p + "block2.project.bias": 0.1 * r(c, seed=8)}
    if cin != c:
        sd[p + "to_out.weight"] = r(c, cin, 1, seed=9, scale=cin ** -0.5)
        sd[p + "to_out.bias"] = 0.1 * r(c, seed=10)
    return sd


FILM_OFF = 64          # SHR offset of the ResNet blocks' FiLM rows in the two chain programs below


def resnets_in_tf128(kind, T, B, n_res, layers, cross, prod, x=None, sk=None, sd_edit=None):
    """MDT_OP_TF128 with MDT_F_RES_KIND 1 / 2 (test_resnet_blocks_inside_the_transformer_launch): ResnetBlock1d blocks of the
    128-channel level in front of the transformer, one launch.  Per-sample arena: [x | y | skip 0 .. n_res-1 | K/V layers].
    sd_edit(sd): changes the seeded parameters before they are compiled."""
    from moleculediffusiontransformer_amd.compiler import Ten, UNetCompiler
    from moleculediffusiontransformer_amd.netspec import inverse_unet_config
    C, n_ctx, mid, G = 128, 12, 512, 8
    cfg = inverse_unet_config(16, 64, 128, n_ctx)
    p = "tf."
    sd = transformer_sd(p, C, max(layers, 1), cross)
    blocks = [f"res{k}." for k in range(n_res)]
    for k, bp in enumerate(blocks):
        sd.update(resnet_sd(bp, C, C if kind == 1 else 2 * C, 100 * (k + 1)))
    if sd_edit is not None:
        sd_edit(sd)
    comp = UNetCompiler(cfg, 64, n_ctx, sd, gemm_mode=prod)
    assert all(comp.res128_ok(bp, C, T, G, kind == 2) for bp in blocks) and comp.tf128_ok(C, T, layers, cross, kind, n_res)
    xt, y = Ten(A, 0, T, C), Ten(A, T * C, T, C)
    skips = [Ten(A, (2 + k) * T * C, T, C) for k in range(n_res)]
    if kind == 2:
        skips = skips[::-1]                  # consumed from the highest address downwards
    comp.transformer_fused128(xt, p, C, layers, cross, False, res=(kind, blocks, G, skips, 2 ** -0.5), y=y)
    op = comp.ops[0]
    assert op.kind == rt.OP_TF128 and len(comp.ops) == 1
    op.p3 = ref(S, FILM_OFF)
    kv_floats = n_ctx * 2 * mid
    if cross:
        op.a2 = ref(A, (2 + n_res) * T * C)
    act_x = _flat(x, rnd(B * T * C, seed=13) * 1.5 + 0.3)
    sk_in = _flat(sk, rnd(n_res * B * T * C, seed=16) * 1.2 - 0.1) if kind == 2 else torch.zeros(n_res * B * T * C)
    kv_all = rnd(layers * B * kv_floats, seed=14) if cross else torch.zeros(0)
    act = torch.cat([act_x, torch.zeros(B * T * C), sk_in, kv_all])
    shr = torch.cat([torch.zeros(FILM_OFF), 0.3 * rnd(n_res * 2 * C, seed=15), torch.zeros(256)])
    return NS(ops=[op], weights=comp.W.pack(), act=act, shr=shr, ext={}, B=B, sd=sd, p=p, blocks=blocks, C=C, G=G,
              act_x=act_x, sk_in=sk_in, kv_all=kv_all, kv_floats=kv_floats)


def resnet_chain256(kind, T, B, n_res, form, prod, x=None, sk=None, sd_edit=None):
    """MDT_OP_RES256 (test_resnet_chain_256): a chain of ResnetBlock1d blocks of a 256-channel level in one launch, whole or
    pair-split.  Per-sample arena: [x | y | skip 0 .. n_res-1].  Needs MDT_RES256=1 in the environment while it compiles."""
    from moleculediffusiontransformer_amd.compiler import Ten, UNetCompiler
    from moleculediffusiontransformer_amd.netspec import inverse_unet_config
    C, G = 256, 8
    cfg = inverse_unet_config(16, 64, 128, 12)
    blocks = [f"res{k}." for k in range(n_res)]
    sd = {}
    for k, bp in enumerate(blocks):
        sd.update(resnet_sd(bp, C, C if kind == 1 else 2 * C, 100 * (k + 1)))
    if sd_edit is not None:
        sd_edit(sd)
    xt, y = Ten(A, 0, T, C), Ten(A, T * C, T, C)
    skips = [Ten(A, (2 + k) * T * C, T, C) for k in range(n_res)]
    if kind == 2:
        skips = skips[::-1]                  # consumed from the highest address downwards

    def compiled(nsplit):
        comp = UNetCompiler(cfg, 64, 12, sd, gemm_mode="f32" if prod == "f32" else "bf16x3")
        assert all(comp.res256_ok(bp, C, T, G, kind == 2) for bp in blocks)
        comp.pair_stride = 1 if form == "pair1" else 8
        comp.resnet_chain256(xt, blocks, kind, skips, 2 ** -0.5, y, False, nsplit=nsplit)
        op = comp.ops[0]
        assert op.kind == rt.OP_RES256 and len(comp.ops) == 1 and op.i[rt.F_NPOST] == (1 if T == 1 else 3)
        op.p3 = ref(S, FILM_OFF)
        return op, comp.W.pack()
    op, weights = compiled(1 if form == "whole" else 2)
    assert op.i[rt.F_NSPLIT] == (0 if form == "whole" else 2)
    ext = {} if form == "whole" else handoff_ext(B, T)
    act_x = _flat(x, rnd(B * T * C, seed=13) * 1.5 + 0.3)
    sk_in = _flat(sk, rnd(n_res * B * T * C, seed=16) * 1.2 - 0.1) if kind == 2 else torch.zeros(n_res * B * T * C)
    act = torch.cat([act_x, torch.zeros(B * T * C), sk_in])
    shr = torch.cat([torch.zeros(FILM_OFF), 0.3 * rnd(n_res * 2 * C, seed=15), torch.zeros(256)])
    return NS(ops=[op], weights=weights, act=act, shr=shr, ext=ext, B=B, sd=sd, blocks=blocks, C=C, G=G, act_x=act_x,
              sk_in=sk_in, unsplit=lambda: compiled(1))
