"""-m gpu: every hand-written softmax of csrc/ (k_attn<1|2|4>, k_attn_long, k_attn_ctx<1|2>, and the self / cross sections of
k_tblock_lw, k_tblock32, k_tf128, k_tf256) at the edges of its range -- logits of +-120 to +-200, maxima that move by 30 per key
chunk, one-hot rows, exactly uniform rows -- against the fp64 closed forms of tests/softmax_ref.py.

The budget is stated once, in softmax_ref.check(): 8 e_ref (+ 4 e16 on a split-bf16 path) + 2e-6 max(1, |R|max), with e_ref and
e16 measured between references.  Every case records max|G - R| / budget; the last test of the file dumps them (DESIGN.md
section 4.1 holds the table).  A ratio above 1 is a finding in the kernel, not a reason to touch a margin."""
import json
import os

import pytest
import torch

import softmax_ref as sr
from gpu_util import run_both
from moleculediffusiontransformer_amd import runtime as rt
from softmax_ref import (ATTN16_CASES, ATTN_SHAPES, CTX_FAMILIES, CTX_SHAPES, GAINS, TBLOCK_CASES, TF_CASES, attn_case,
                         attn_families, attn_refs, ctx_case, ctx_refs, tblock_case, tblock_form, tblock_refs, tf_case, tf_form,
                         tf_refs)

pytestmark = pytest.mark.gpu

RATIOS = {}
F64 = torch.float64


def launch(lowered):
    """The op on the GPU (run_both: and on the interpreter, which this file does not look at): its result in the shape of R
    and the ext buffers; the input ranges of the arena must come back bit for bit."""
    ops, weights, act, shr, ext, B, out, untouched = lowered
    (ga, _, ge), _ = run_both(ops, weights, act, shr, ext, B)
    for lo, hi in untouched:
        assert torch.equal(ga[lo:hi], act[lo:hi]), "an input was written"
    return out(ga), ge


def record(key, G, refs, split, R=None):
    assert torch.isfinite(G).all()
    r = sr.ratio(G, refs, split, R)
    RATIOS[key] = dict(smax=round(refs.smax, 1), e_ref=refs.e_ref, e16=refs.e16, ratio=round(r, 4))
    print(f"\n{key}: |s|max {refs.smax:.1f} e_ref {refs.e_ref:.3g} e16 {refs.e16:.3g} ratio {r:.3f}")
    return sr.check(G, refs, split, R)


# ---- MDT_OP_ATTN -----------------------------------------------------------------------------------------------------------------

def attn_properties(G, c, out16=0):
    T, Tk = c["q"].shape[1], c["k"].shape[1]
    if c["family"] == "onehot":
        # the winner leads by 60: every other weight is below e^-60, the row IS the winner's value row
        want = torch.gather(c["v"], 1, c["win"].unsqueeze(-1).expand(-1, -1, -1, sr.D))
        if out16:
            assert torch.equal(G, want.to(torch.bfloat16).float())
        else:
            assert ((G.double() - want.double()).abs() <= sr.ulp32(want)).all()
    return c["v"].double().mean(1, keepdim=True).expand(-1, T, -1, -1) if c["family"] == "flat" else None


@pytest.mark.parametrize("kernel,B,T,Tk,family", [s + (f,) for s in ATTN_SHAPES for f in attn_families(s[3])])
def test_attention_range(kernel, B, T, Tk, family):
    c, refs = attn_case(B, T, Tk, family), attn_refs(B, T, Tk, family)
    G, _ = launch(sr.lower_attn(c))
    record(f"{kernel} ({T},{Tk}) {family} f32", G, refs, False)
    mean = attn_properties(G, c)
    if mean is not None:                # exactly the sample's own Tk keys, none of the tile's padding
        sr.check(G, refs, False, mean)


@pytest.mark.parametrize("family", ["hot", "onehot"])
@pytest.mark.parametrize("kernel,B,T,Tk,in16,out16,merged", ATTN16_CASES)
def test_attention_range_with_bf16_operands(kernel, B, T, Tk, in16, out16, merged, family):
    """q and / or k | v as bf16 (the merged q | k | v tensor where all three are): the reference on the exactly widened values; a
    bf16 output against R rounded to bf16, one bf16 ulp."""
    c, refs = attn_case(B, T, Tk, family, in16), attn_refs(B, T, Tk, family, in16)
    G, _ = launch(sr.lower_attn(c, in16, out16, merged))
    key = f"{kernel} ({T},{Tk}) in16={in16} out16={out16} {family} f32"
    if out16:
        assert torch.isfinite(G).all()
        off = ((G.double() - refs.R.to(torch.bfloat16).double()).abs() / sr.ulp16(refs.R)).max().item()
        RATIOS[key] = dict(smax=round(refs.smax, 1), e_ref=refs.e_ref, e16=refs.e16, bf16_ulps=off)
        assert off <= 1.0
    else:
        record(key, G, refs, False)
    attn_properties(G, c, out16)


# ---- MDT_OP_ATTN_CTX -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("split", [0, 1])            # (varies fastest: both product modes of a case share its references)
@pytest.mark.parametrize("family", CTX_FAMILIES)
@pytest.mark.parametrize("kernel,B,T,Tk", CTX_SHAPES)
def test_context_attention_range(kernel, B, T, Tk, split, family):
    c, refs = ctx_case(B, T, Tk, family), ctx_refs(B, T, Tk, family)
    G, _ = launch(sr.lower_ctx(c, T, split))
    record(f"{kernel} B={B} ({T},{Tk}) {family} {'bf16x3' if split else 'f32'}", G, refs, bool(split))
    if family == "onehot":
        want = torch.gather(c["c"], 1, c["win"].unsqueeze(-1).expand(-1, -1, sr.F_CTX))
        assert ((G.double() - want.double()).abs() <= sr.ulp32(want)).all()
    if family == "flat":
        sr.check(G, refs, bool(split), c["c"].double().mean(1, keepdim=True).expand(-1, T * sr.H, -1))


# ---- the fused kernels -----------------------------------------------------------------------------------------------------------

MODE = {rt.TB_SELF: "self", rt.TB_CROSS: "cross"}


@pytest.mark.parametrize("prod", ["bf16x3", "f32"])
@pytest.mark.parametrize("gain", GAINS + [-32])
@pytest.mark.parametrize("kernel,variant,mode,C,T,B", TBLOCK_CASES)
def test_sub_block_range(kernel, variant, mode, C, T, B, gain, prod):
    """MDT_OP_TBLOCK: the -INFINITY masks of its softmax sections cover the padded keys and the keys of the other samples of a
    16-row tile; at gain 0 every row must be the mean over exactly its sample's own keys."""
    c, refs = tblock_case(variant, mode, C, T, B), tblock_refs(variant, mode, C, T, B, gain)
    G, _ = launch(sr.lower_tblock(c, gain, prod))
    record(f"{kernel} v{variant} {MODE[mode]} ({C},{T},{B}) gain {gain} {prod}", G, refs, prod == "bf16x3")
    if gain == 0:
        sr.check(G, refs, prod == "bf16x3", tblock_form(c, gain, sr.uniform)(F64, sr.ident))


TF_PARAMS = [case[:6] + (g, form)
             for case in TF_CASES for g in case[6] for form in (("whole",) if case[1] == 128 else ("whole", "pair8", "pair1"))]


@pytest.mark.parametrize("prod", ["bf16x3", "f32"])
@pytest.mark.parametrize("kernel,C,T,B,layers,cross,gain,form", TF_PARAMS)
def test_transformer_range(kernel, C, T, B, layers, cross, gain, form, prod):
    """MDT_OP_TF128 / MDT_OP_TF256, whole and pair-split (the hand-off flag words as test_gpu_ops.test_fused_transformer)."""
    c, refs = tf_case(C, T, B, layers, cross), tf_refs(C, T, B, layers, cross, gain)
    G, ge = launch(sr.lower_tf(c, gain, prod, form))
    if form != "whole":
        flags = ge[3].view(torch.int32)
        assert int(flags[0]) == 0, "a hand-off poll timed out"
        assert bool((flags[64::32] == 1 + layers * (3 if cross else 2)).all()), "one hand-off per sub-block and (row block, half)"
    record(f"{kernel} {form} ({C},{T},{B}) layers {layers} {'cross' if cross else 'self'} gain {gain} {prod}", G, refs,
           prod == "bf16x3")
    if gain == 0:
        sr.check(G, refs, prod == "bf16x3", tf_form(c, gain, sr.uniform)(F64, sr.ident))


def test_zz_dump_ratios():
    """Last in the file: every ratio the run recorded, as one JSON object (shown under -s; written to the file that
    MDT_SOFTMAX_RATIOS names), and its largest per product mode.  A recorder: each case asserts its own ratio."""
    text = json.dumps(RATIOS, indent=0, sort_keys=True)
    print("\n" + text)
    if os.environ.get("MDT_SOFTMAX_RATIOS"):
        with open(os.environ["MDT_SOFTMAX_RATIOS"], "w") as f:
            f.write(text)
    for mode in ("f32", "bf16x3"):
        rs = [v["ratio"] for k, v in RATIOS.items() if k.endswith(mode) and "ratio" in v]
        if rs:
            print(f"largest ratio, {mode}: {max(rs):.3f} over {len(rs)} cases")
