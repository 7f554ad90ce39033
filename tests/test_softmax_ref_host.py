"""CPU: tests/softmax_ref.py is a fit yardstick for tests/test_gpu_softmax_range.py -- its fp32 closed forms are the operators that
oracle/program_interp.py interprets, its input families have the properties they claim, its budget rejects a softmax that
does not subtract the maximum, a mask that leaks and an online softmax that does not rescale, and no budget is loose."""
import pytest
import torch

import softmax_ref as sr
from oracle.program_interp import Buffers, run_program
from softmax_ref import (ATTN16_CASES, ATTN_SHAPES, CTX_SHAPES, GAINS, TBLOCK_CASES, TF_CASES, attn_case, attn_families, attn_ref,
                         attn_refs, ctx_case, ctx_ref, ctx_refs, tblock_case, tblock_form, tblock_refs, tf_case, tf_form, tf_refs)

F32, H_ = torch.float32, sr.H


def interp(lowered):
    ops, weights, act, shr, ext, B, out, _ = lowered
    bufs = Buffers(weights.clone(), act.clone(), shr.clone(), {k: v.clone().view(-1) for k, v in ext.items()})
    run_program(ops, bufs, B, 0)
    return out(bufs.act)


def rejected(G, refs, split):
    try:
        sr.check(G, refs, split)
    except AssertionError:
        return True
    return False


# ---- 1. the closed forms are the interpreter's operators -------------------------------------------------------------------------

@pytest.mark.parametrize("kernel,B,T,Tk", ATTN_SHAPES)
def test_attn_closed_form_is_the_interpreters_op(kernel, B, T, Tk):
    c = attn_case(B, T, Tk, "benign")
    assert (interp(sr.lower_attn(c)) - attn_refs(B, T, Tk, "benign").I).abs().max() < 1e-5


@pytest.mark.parametrize("kernel,B,T,Tk,in16,out16,merged", ATTN16_CASES)
def test_attn_bf16_closed_form_is_the_interpreters_op(kernel, B, T, Tk, in16, out16, merged):
    c = attn_case(B, T, Tk, "benign", in16)
    got, want = interp(sr.lower_attn(c, in16, out16, merged)), attn_refs(B, T, Tk, "benign", in16).I
    if out16:           # both round the same fp32 value up to summation order: equal, or one bf16 ulp apart at a tie
        assert ((got - want.to(torch.bfloat16).float()).abs() <= sr.ulp16(want)).all()
    else:
        assert (got - want).abs().max() < 1e-5


@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("kernel,B,T,Tk", CTX_SHAPES)
def test_ctx_closed_form_is_the_interpreters_op(kernel, B, T, Tk, split):
    c = ctx_case(B, T, Tk, "benign")
    assert (interp(sr.lower_ctx(c, T, split)) - ctx_refs(B, T, Tk, "benign").I).abs().max() < 1e-5


@pytest.mark.parametrize("kernel,variant,mode,C,T,B", TBLOCK_CASES)
def test_subblock_closed_form_is_the_interpreters_op(kernel, variant, mode, C, T, B):
    # exact-fp32 weight tiles: the interpreter then differs from the closed form by the folding of LayerNorm's gain and
    # the summation order alone
    got = interp(sr.lower_tblock(tblock_case(variant, mode, C, T, B), 1, "f32"))
    assert (got - tblock_refs(variant, mode, C, T, B, 1).I).abs().max() < 1e-5


# (the pair split exists for the 256-channel level only)
@pytest.mark.parametrize("kernel,C,T,B,layers,cross,gains,form",
                         [c + (f,) for c in TF_CASES for f in (("whole",) if c[1] == 128 else ("whole", "pair8"))])
def test_transformer_closed_form_is_the_interpreters_op(kernel, C, T, B, layers, cross, gains, form):
    c, refs = tf_case(C, T, B, layers, cross), tf_refs(C, T, B, layers, cross, 1)
    diff = (interp(sr.lower_tf(c, 1, "f32", form)) - refs.I).abs().max().item()
    if (C, layers) == (256, 2):
        # two layers of 256 channels with cross-attention: I itself is 7.0e-6 from R here (e_ref) and the output reaches 10, so
        # two fp32 evaluations of the operator stand up to 2 e_ref = 1.4e-5 apart; measured 1.05e-5, held to 2e-5 -- and to
        # the budget of the exact-product kernels at the gain the case runs with
        assert diff < 2e-5 and 2 * refs.e_ref < 2e-5
        sr.check(interp(sr.lower_tf(c, gains[0], "f32", form)), tf_refs(C, T, B, layers, cross, gains[0]), False)
    else:
        assert diff < 1e-5


# ---- 2. the families are what they claim -----------------------------------------------------------------------------------------

def lead(logits, win):
    """Smallest distance of a row's winner to every other key of the row."""
    top = torch.gather(logits, -1, win.unsqueeze(-1))
    others = logits.scatter(-1, win.unsqueeze(-1), float("-inf"))
    return (top - others.amax(-1, keepdim=True)).min().item()


@pytest.mark.parametrize("kernel,B,T,Tk,in16", [s + (0,) for s in ATTN_SHAPES] + [c[:4] + (c[4],) for c in ATTN16_CASES])
def test_attn_onehot_winner_leads_by_60_and_covers_the_tile_edges(kernel, B, T, Tk, in16):
    c = attn_case(B, T, Tk, "onehot", in16)
    win = c["win"].permute(0, 2, 1)                                            # [B, H, T] as the logits
    assert lead(c["logits"], win) >= 60
    chunk = 64 if Tk > 64 else 16
    want = {j for j in (0, 15, 16, Tk - 1, 63, 64, (Tk - 1) // chunk * chunk) if 0 <= j < Tk}
    assert want == set(c["listed"]) and want <= set(win.reshape(-1).tolist())
    assert torch.equal(win.reshape(-1)[len(c["listed"]):], ((7 * torch.arange(B * H_ * T) + 3) % Tk)[len(c["listed"]):])


@pytest.mark.parametrize("kernel,B,T,Tk", CTX_SHAPES)
def test_ctx_onehot_winner_leads_by_60_and_covers_the_chunk_edges(kernel, B, T, Tk):
    c = ctx_case(B, T, Tk, "onehot")
    assert lead(c["logits"], c["win"]) >= 60
    want = {j for j in (0, 15, 16, Tk - 1, 63, 64, (Tk - 1) // 16 * 16) if 0 <= j < Tk}
    assert want == set(c["listed"]) and want <= set(c["win"].reshape(-1).tolist())


@pytest.mark.parametrize("kernel,B,T,Tk", ATTN_SHAPES)
def test_attn_shift_moves_the_logits_by_150_and_nothing_else(kernel, B, T, Tk):
    c = attn_case(B, T, Tk, "shift")
    moved = c["logits"] - sr.attn_logits(c["q"], c["k0"], c["scale"])
    sign = torch.where(torch.arange(T) % 2 == 0, 1.0, -1.0).double().view(1, 1, T, 1)
    assert (moved - 150 * sign).abs().max() < 1e-9
    assert (c["logits"].abs().amin(-1) > 130).all() and c["logits"].abs().max() < 175
    assert (attn_ref(c["q"], c["k"], c["v"], c["scale"]) - attn_ref(c["q"], c["k0"], c["v"], c["scale"])).abs().max() < 1e-9


@pytest.mark.parametrize("kernel,B,T,Tk", CTX_SHAPES)
def test_ctx_shift_moves_the_logits_by_150_and_the_output_by_the_offset(kernel, B, T, Tk):
    c = ctx_case(B, T, Tk, "shift")
    moved = c["logits"] - sr.ctx_logits(c["q"], c["c0"], c["scale"])
    sign = torch.where(torch.arange(T * H_) % 2 == 0, 1.0, -1.0).double().view(1, -1, 1)
    assert (moved - 150 * sign).abs().max() < 1e-9
    assert (ctx_ref(c["q"], c["c"], c["scale"]) - c["u"].double() - ctx_ref(c["q"], c["c0"], c["scale"])).abs().max() < 1e-9


@pytest.mark.parametrize("kernel,B,T,Tk", ATTN_SHAPES)
def test_attn_flat_is_the_mean_of_the_value_rows(kernel, B, T, Tk):
    c = attn_case(B, T, Tk, "flat")
    assert c["logits"].abs().max() == 0
    mean = c["v"].double().mean(1, keepdim=True).expand(-1, T, -1, -1)
    assert (attn_refs(B, T, Tk, "flat").R - mean).abs().max() < 1e-12


@pytest.mark.parametrize("kernel,B,T,Tk", CTX_SHAPES)
def test_ctx_flat_is_the_mean_of_the_context_rows(kernel, B, T, Tk):
    c = ctx_case(B, T, Tk, "flat")
    assert c["logits"].abs().max() == 0
    assert (ctx_refs(B, T, Tk, "flat").R - c["c"].double().mean(1, keepdim=True)).abs().max() < 1e-12


@pytest.mark.parametrize("kernel,B,T,Tk", [s for s in ATTN_SHAPES if s[3] > 64])
@pytest.mark.parametrize("family", ["stairs_up", "stairs_down"])
def test_stairs_chunk_maxima_step_by_30(kernel, B, T, Tk, family):
    s = attn_case(B, T, Tk, family)["logits"]
    top = torch.stack([c.amax(-1) for c in s.split(64, -1)], -1)
    step = top[..., 1:] - top[..., :-1]
    assert ((step - (30 if family == "stairs_up" else -30)).abs() <= 8).all()


def test_hot_logits_span_120():
    for _, B, T, Tk in ATTN_SHAPES:
        assert 75 < attn_case(B, T, Tk, "hot")["logits"].abs().max() < 200


@pytest.mark.parametrize("kernel,variant,mode,C,T,B", TBLOCK_CASES)
def test_gains_set_the_logit_range_of_a_sub_block(kernel, variant, mode, C, T, B):
    assert tblock_refs(variant, mode, C, T, B, 0).smax == 0
    assert 25 < tblock_refs(variant, mode, C, T, B, 8).smax < 60
    assert 100 < tblock_refs(variant, mode, C, T, B, 32).smax < 240
    assert tblock_refs(variant, mode, C, T, B, -32).smax == tblock_refs(variant, mode, C, T, B, 32).smax


# ---- 3. the budget discriminates, 4. and is capped -------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel,B,T,Tk", ATTN_SHAPES)
def test_attn_budget_rejects_wrong_softmaxes(kernel, B, T, Tk):
    def wrong(family, sm, in16=0):
        c = attn_case(B, T, Tk, family, in16)
        return attn_ref(c["q"], c["k"], c["v"], c["scale"], F32, softmax=sm)
    for family in attn_families(Tk):
        refs, top = attn_refs(B, T, Tk, family), attn_case(B, T, Tk, family)["logits"].max()
        assert sr.cap_holds(refs, False), family
        assert not rejected(refs.I, refs, False)
        if family in ("hot", "shift", "onehot") or (family == "stairs_up" and Tk > 192):
            assert top > sr.EXP_MAX
        if top > sr.EXP_MAX:
            assert rejected(wrong(family, sr.naive), refs, False), family
        if family in ("flat", "onehot"):
            assert rejected(wrong(family, sr.leaky), refs, False), family
        if family == "stairs_up":
            assert rejected(wrong(family, sr.online_alpha1), refs, False)
    refs = attn_refs(B, T, Tk, "benign")
    assert sr.cap_holds(refs, False) and not rejected(wrong("benign", sr.naive), refs, False)


@pytest.mark.parametrize("kernel,B,T,Tk,in16,out16,merged", ATTN16_CASES)
def test_attn_bf16_budget_rejects_wrong_softmaxes(kernel, B, T, Tk, in16, out16, merged):
    for family in ("hot", "onehot"):
        c, refs = attn_case(B, T, Tk, family, in16), attn_refs(B, T, Tk, family, in16)
        assert sr.cap_holds(refs, False)
        assert rejected(attn_ref(c["q"], c["k"], c["v"], c["scale"], F32, softmax=sr.naive), refs, False), family


@pytest.mark.parametrize("kernel,B,T,Tk", CTX_SHAPES)
def test_ctx_budget_rejects_wrong_softmaxes(kernel, B, T, Tk):
    def wrong(family, sm):
        c = ctx_case(B, T, Tk, family)
        return ctx_ref(c["q"], c["c"], c["scale"], F32, softmax=sm)
    for family in sr.CTX_FAMILIES:
        refs, top = ctx_refs(B, T, Tk, family), ctx_case(B, T, Tk, family)["logits"].max()
        assert sr.cap_holds(refs, True), family
        assert not rejected(refs.I, refs, False)
        # against the wider of the two budgets (split-bf16 scores): rejected there, rejected by both
        if family in ("hotter", "shift", "onehot"):
            assert top > sr.EXP_MAX
        if top > sr.EXP_MAX:
            assert rejected(wrong(family, sr.naive), refs, True), family
        if family in ("flat", "onehot"):
            assert rejected(wrong(family, sr.leaky), refs, True), family
    refs = ctx_refs(B, T, Tk, "benign")
    assert sr.cap_holds(refs, True) and not rejected(wrong("benign", sr.naive), refs, False)


@pytest.mark.parametrize("kernel,variant,mode,C,T,B", TBLOCK_CASES)
def test_subblock_budget_rejects_wrong_softmaxes(kernel, variant, mode, C, T, B):
    c = tblock_case(variant, mode, C, T, B)
    for gain in GAINS + [-32]:
        refs = tblock_refs(variant, mode, C, T, B, gain)
        assert sr.cap_holds(refs, True), gain
        assert not rejected(refs.I, refs, False)
        if abs(gain) == 32:
            assert refs.smax > sr.EXP_MAX
            assert rejected(tblock_form(c, gain, sr.naive)(F32, sr.ident), refs, True), gain
        if gain == 0:
            assert rejected(tblock_form(c, gain, sr.leaky)(F32, sr.ident), refs, True)
    refs = tblock_refs(variant, mode, C, T, B, 1)
    assert sr.cap_holds(refs, True) and not rejected(tblock_form(c, 1, sr.naive)(F32, sr.ident), refs, False)


@pytest.mark.parametrize("kernel,C,T,B,layers,cross,gains", TF_CASES)
def test_transformer_budget_rejects_wrong_softmaxes(kernel, C, T, B, layers, cross, gains):
    c = tf_case(C, T, B, layers, cross)
    for gain in gains:
        refs = tf_refs(C, T, B, layers, cross, gain)
        assert sr.cap_holds(refs, True), gain
        assert not rejected(refs.I, refs, False)
        if gain == 32:
            assert refs.smax > sr.EXP_MAX
            assert rejected(tf_form(c, gain, sr.naive)(F32, sr.ident), refs, True)
        if gain == 0:
            assert rejected(tf_form(c, gain, sr.leaky)(F32, sr.ident), refs, True)
    refs = tf_refs(C, T, B, layers, cross, 1)
    assert sr.cap_holds(refs, True) and not rejected(tf_form(c, 1, sr.naive)(F32, sr.ident), refs, False)


def test_split_operand_drops_about_2_to_the_minus_18():
    x = sr.rnd(4096, seed=7).double() * 3
    rel = ((sr.r16(x) - x).abs() / x.abs()).max().item()
    assert 2.0 ** -19 < rel <= 2.0 ** -16
