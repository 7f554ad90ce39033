"""-m gpu: the block form of k_tf256's cross-attention core (4-token samples: per-sample 4 x 4 x 1 MFMA blocks instead of 16 x 16
tiles over the wave's 16 rows).  One MDT_OP_TF256 op, C = 256, T = 4, against the CPU interpreter and the module arithmetic at the
op's own tolerance, 2e-4 * max(1, |y|max).

The dimensions -- batch sizes 1, 5, 8, 9, 37 (4 rows: less than a row tile; 20: a ragged second tile; 32: exactly one block; one
block plus one sample; several blocks with a ragged end), context lengths 12, 9, 3 (three key groups; a partly filled last group;
one group), per-sample and shared K/V rows, 1 and 2 layers with and without cross-attention, the whole and the pair-split form,
both product types -- are covered pairwise rather than as a 480-case product: every batch size in every form and product type at
the headline's context length; every other context length with both K/V sources in every form and product type at the batch that
crosses a block; the shared rows at the headline's context length; the self-only transformer in both depths."""
import pytest
import torch
import torch.nn.functional as F

from gpu_util import ref, rnd, run_both
from moleculediffusiontransformer_amd import runtime as rt
from test_gpu_ops import _handoff_ext, _transformer_sd, prod  # noqa: F401  (prod: the product-type fixture)

pytestmark = pytest.mark.gpu

A, S = rt.SP_ACT, rt.SP_SHR
C, T, MID, H = 256, 4, 512, 8


def _build(n_ctx, layers, cross, shared, form):
    from moleculediffusiontransformer_amd.compiler import Ten, UNetCompiler
    from moleculediffusiontransformer_amd.netspec import inverse_unet_config
    sd = _transformer_sd("tf.", C, layers, cross)
    comp = UNetCompiler(inverse_unet_config(16, 64, 128, n_ctx), 64, n_ctx, sd, tf256=(form == "whole"))
    comp.pair_stride = 8
    comp.transformer(Ten(A, 0, T, C), "tf.", C, layers, cross, free_input=False)
    assert [o.kind for o in comp.ops] == [rt.OP_TF256]
    op = comp.ops[0]
    assert op.i[rt.F_NSPLIT] == (1 if form == "whole" else 2)
    op.out = ref(A, T * C)
    if cross:
        if shared:
            op.a2 = ref(S, 0)
            op.i[rt.F_KV_BSTRIDE] = 0
        else:
            op.a2 = ref(A, 2 * T * C)
    return sd, comp, op


def _module(sd, x, kv, layers, cross):
    """Transformer1d (modules.py:469-524) written out with torch ops; kv: [layer][B, n_ctx, 2 mid] projected context rows."""
    B = x.shape[0]
    p = "tf."

    def attn(q_, x_, kv_=None):
        xn = F.layer_norm(x_, (C,), sd[q_ + "norm.weight"], sd[q_ + "norm.bias"], 1e-5)
        qq = (xn @ sd[q_ + "to_q.weight"].T).view(B, T, H, 64).transpose(1, 2)
        if kv_ is None:
            cn = F.layer_norm(x_, (C,), sd[q_ + "norm_context.weight"], sd[q_ + "norm_context.bias"], 1e-5)
            kv_ = cn @ sd[q_ + "to_kv.weight"].T
        k_, v_ = kv_.chunk(2, dim=-1)
        k_ = k_.reshape(B, -1, H, 64).transpose(1, 2)
        v_ = v_.reshape(B, -1, H, 64).transpose(1, 2)
        o = ((qq @ k_.transpose(-1, -2)) * 0.125).softmax(-1) @ v_
        return o.transpose(1, 2).reshape(B, T, MID) @ sd[q_ + "attention.to_out.weight"].T + sd[q_ + "attention.to_out.bias"]
    h = F.group_norm(x.transpose(1, 2), 32, sd[p + "to_in.0.weight"], sd[p + "to_in.0.bias"], 1e-6)
    h = F.conv1d(h, sd[p + "to_in.1.weight"], sd[p + "to_in.1.bias"]).transpose(1, 2)
    for li in range(layers):
        bp = p + f"blocks.{li}."
        h = h + attn(bp + "attention.", h)
        if cross:
            h = h + attn(bp + "cross_attention.", h, kv[li])
        f_ = bp + "feed_forward."
        h = h + F.gelu(h @ sd[f_ + "0.weight"].T + sd[f_ + "0.bias"]) @ sd[f_ + "2.weight"].T + sd[f_ + "2.bias"]
    return F.conv1d(h.transpose(1, 2), sd[p + "to_out.1.weight"], sd[p + "to_out.1.bias"]).transpose(1, 2)


CASES = (
    # every batch size at the headline's context length, per-sample K/V rows, 2 layers
    [(B, 12, False, 2, True) for B in (1, 5, 8, 9, 37)]
    # the other context lengths with both K/V sources, across a block boundary
    + [(9, n_ctx, shared, 1, True) for n_ctx in (9, 3) for shared in (False, True)]
    # shared rows at the headline's context length, several blocks
    + [(37, 12, True, 1, True)]
    # no cross-attention: the launch without K/V tiles, both depths
    + [(9, 12, False, 1, False), (5, 12, False, 2, False)])


@pytest.mark.parametrize("form", ["whole", "pair8"])
@pytest.mark.parametrize("B,n_ctx,shared,layers,cross", CASES)
def test_tf256_four_token_samples(B, n_ctx, shared, layers, cross, form, prod):
    """The op against the CPU interpreter and the module arithmetic; the launch's own selection function names the block core
    for it; the same launch again from the same buffers returns the same bits; the hand-off status word stays 0."""
    sd, comp, op = _build(n_ctx, layers, cross, shared, form)
    assert op.i[rt.F_T] == T and op.i[rt.F_WF32] == int(prod == "f32")
    assert rt.load_library().mdt_tf256_block_core(op.i[rt.F_T], op.i[rt.F_TK], op.i[rt.F_CROSS]) == int(cross)
    if cross:
        assert op.i[rt.F_TK] == n_ctx
    ext = _handoff_ext(B, T) if form != "whole" else {}
    kv_floats = n_ctx * 2 * MID
    act_x = rnd(B * T * C, seed=13) * 1.5 + 0.3
    kv_all = rnd(layers * B * kv_floats, seed=14) if cross and not shared else torch.zeros(0)
    shr = rnd(layers * kv_floats, seed=15) if cross else torch.zeros(4)
    act = torch.cat([act_x, torch.zeros(B * T * C), kv_all])
    W = comp.W.pack()
    (ga, _, ge), (ca, _, _) = run_both([op], W, act, shr, ext, B)
    yg, yc = ga[B * T * C: 2 * B * T * C].view(B, T, C), ca[B * T * C: 2 * B * T * C].view(B, T, C)
    assert torch.isfinite(yg).all()
    if ext:
        flags = ge[3].view(torch.int32)
        assert int(flags[0]) == 0, "a hand-off poll timed out"
        assert bool((flags[64::32] == 1 + layers * (3 if cross else 2)).all())
    if cross and shared:
        kv = [shr[li * kv_floats: (li + 1) * kv_floats].view(1, n_ctx, 2 * MID).expand(B, -1, -1) for li in range(layers)]
    elif cross:
        kv = [kv_all[li * B * kv_floats: (li + 1) * B * kv_floats].view(B, n_ctx, 2 * MID) for li in range(layers)]
    else:
        kv = None
    want = _module(sd, act_x.view(B, T, C), kv, layers, cross)
    tol = 2e-4 * max(1.0, yc.abs().max().item())
    e_int, e_mod = (yg - yc).abs().max().item(), (yg - want).abs().max().item()
    print(f"tf256 T=4 B={B} ctx={n_ctx} shared={int(shared)} layers={layers} cross={int(cross)} {form} {prod}: "
          f"max|gpu - interpreter| = {e_int:.3e}, max|gpu - module| = {e_mod:.3e}, tolerance {tol:.3e}")
    assert e_int < tol, e_int
    assert e_mod < tol, e_mod
    assert torch.equal(ga[: B * T * C], act_x) and torch.equal(ga[2 * B * T * C:], kv_all)     # inputs untouched
    (ga2, _, _), _ = run_both([op], W, act, shr, ext, B)
    assert torch.equal(ga2, ga)


@pytest.mark.parametrize("form", ["whole", "pair8"])
@pytest.mark.parametrize("n_ctx", [12, 9])
def test_tf256_block_core_is_position_invariant(n_ctx, form, prod):
    """B = 9: the rows and K/V rows of sample 0 copied to positions 3 and 8 -- another lane quad of the same MFMA, another row tile,
    another workgroup.  The three samples' output rows must be bitwise equal: a block form that leaks between the 16 blocks of
    an instruction, or between the lane quads of an exchange, fails here."""
    B, layers = 9, 2
    sd, comp, op = _build(n_ctx, layers, True, False, form)
    ext = _handoff_ext(B, T) if form != "whole" else {}
    kv_floats = n_ctx * 2 * MID
    x = (rnd(B * T * C, seed=23) * 1.5 + 0.3).view(B, T * C)
    kv = rnd(layers * B * kv_floats, seed=24).view(layers, B, kv_floats)
    for b in (3, 8):
        x[b] = x[0]
        kv[:, b] = kv[:, 0]
    act = torch.cat([x.reshape(-1), torch.zeros(B * T * C), kv.reshape(-1)])
    (ga, _, _), (ca, _, _) = run_both([op], comp.W.pack(), act, torch.zeros(4), ext, B)
    yg, yc = ga[B * T * C: 2 * B * T * C].view(B, T * C), ca[B * T * C: 2 * B * T * C].view(B, T * C)
    assert (yg - yc).abs().max() < 2e-4 * max(1.0, yc.abs().max().item())
    assert torch.equal(yg[3], yg[0]) and torch.equal(yg[8], yg[0])
    assert not torch.equal(yg[1], yg[0])


def test_tf256_core_selection():
    """The launch-selection function itself: the block core for cross-attention at T = 4 with 1..12 context rows, the tile core
    for every other T (the shapes of test_fused_transformer) and for launches without cross-attention."""
    lib = rt.load_library()
    for tk in range(1, 13):
        assert lib.mdt_tf256_block_core(4, tk, 1) == 1
        assert lib.mdt_tf256_block_core(4, tk, 0) == 0
    for t in (1, 2, 8, 16):
        for tk in (3, 9, 12):
            assert lib.mdt_tf256_block_core(t, tk, 1) == 0
    assert lib.mdt_tf256_block_core(4, 13, 1) == 0 and lib.mdt_tf256_block_core(4, 0, 1) == 0
