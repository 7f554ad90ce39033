"""-m gpu: the attention cores of k_tf128 (C = 128: a wave's 16-row tile is whole samples).  In the default mode S^T = K Q^T and
O^T = V^T P^T are split-bf16 MFMAs on q, k, v and p rounded to hi + lo (csrc/k_tf128.hip, scores_split / pv_split); the exact mode
keeps the fp32 MFMAs.  One MDT_OP_TF128 op, built as tests/softmax_ref.py builds it, against that file's fp64 closed forms at the
project's budget (softmax_ref.budget: 8 e_ref + 4 e16 + floor in the default mode, 8 e_ref + floor in the exact mode).

Shapes, 12 context rows:
  (T 16, B 5, self)             the second workgroup has one live wave and clamped rows
  (T 4, B 16), (T 4, B 17)      four samples per tile, the key mask between samples, a tile with one sample
  (T 8, B 3)                    two samples per tile, ragged
  (T 16, B 3, cross)            12 live keys of 16
  (T 16, B 5, self, 2 layers), (T 16, B 3, cross, 2 layers)    chaining through a second layer
Gains 0, 8, 32 on the one-layer shapes, 8 on the two-layer shapes."""
import json
import os

import pytest
import torch

import softmax_ref as sr
from gpu_util import run_both
from softmax_ref import GAINS, tf_case, tf_form, tf_refs

pytestmark = pytest.mark.gpu

C = 128
# (T, B, layers, cross, gains)
SHAPES = [(16, 5, 1, False, GAINS), (4, 16, 1, False, GAINS), (4, 17, 1, False, GAINS), (8, 3, 1, False, GAINS),
          (16, 3, 1, True, GAINS), (16, 5, 2, False, [8]), (16, 3, 2, True, [8])]
PARAMS = [s[:4] + (g,) for s in SHAPES for g in s[4]]
RATIOS = {}


def launch(lowered):
    """The op on the GPU: its result in the shape of R; the input ranges of the arena come back bit for bit."""
    ops, weights, act, shr, ext, B, out, untouched = lowered
    (ga, _, _), _ = run_both(ops, weights, act, shr, ext, B)
    for lo, hi in untouched:
        assert torch.equal(ga[lo:hi], act[lo:hi]), "an input was written"
    return out(ga)


def sub_case(c, lo, hi):
    """Samples lo .. hi - 1 of a case as a batch of their own."""
    B, T, layers = c["B"], c["T"], c["layers"]
    x = c["x"].view(B, T * C)[lo:hi].reshape(-1)
    kv = c["kv"].view(layers, B, -1)[:, lo:hi].reshape(-1) if c["cross"] else c["kv"]
    return dict(c, x=x, kv=kv, B=hi - lo)


def test_no_case_is_left_out():
    """The cap of softmax_ref (margins over the reference's own errors under 5e-3 of the output's scale) holds for every
    (shape, gain) in both modes, so every case below runs."""
    for T, B, layers, cross, gain in PARAMS:
        refs = tf_refs(C, T, B, layers, cross, gain)
        for split in (True, False):
            assert sr.cap_holds(refs, split), (T, B, layers, cross, gain, split, refs.e_ref, refs.e16)


@pytest.mark.parametrize("prod", ["bf16x3", "f32"])          # (varies fastest: both modes of a case share its references)
@pytest.mark.parametrize("T,B,layers,cross,gain", PARAMS)
def test_tf128_core(T, B, layers, cross, gain, prod):
    split = prod == "bf16x3"
    c, refs = tf_case(C, T, B, layers, cross), tf_refs(C, T, B, layers, cross, gain)
    assert sr.cap_holds(refs, split)
    lowered = sr.lower_tf(c, gain, prod)
    G = launch(lowered)
    assert torch.isfinite(G).all()
    r = sr.ratio(G, refs, split)
    key = f"k_tf128 ({T},{B}) layers {layers} {'cross' if cross else 'self'} gain {gain} {prod}"
    RATIOS[key] = dict(smax=round(refs.smax, 1), e_ref=refs.e_ref, e16=refs.e16, ratio=round(r, 4))
    print(f"\n{key}: |s|max {refs.smax:.1f} e_ref {refs.e_ref:.3g} e16 {refs.e16:.3g} budget {sr.budget(refs, split):.3g} "
          f"ratio {r:.3f}")
    sr.check(G, refs, split)
    if gain == 0:                       # the mean over exactly the sample's own keys
        sr.check(G, refs, split, tf_form(c, gain, sr.uniform)(torch.float64, sr.ident))
    assert torch.equal(launch(lowered), G), "the same launch twice gives other bits"


@pytest.mark.parametrize("prod", ["bf16x3", "f32"])
@pytest.mark.parametrize("T,B,cut,cross", [(16, 5, 2, False), (4, 17, 9, False), (16, 3, 2, True)])
def test_tf128_core_is_position_invariant(T, B, cut, cross, prod):
    """The rows of a sample do not depend on where the sample stands: the first `cut` samples and the rest as batches of their own
    (another tile position, another wave, another workgroup, other neighbours in the tile) give the bits of the whole batch."""
    c = tf_case(C, T, B, 1, cross)
    whole = launch(sr.lower_tf(c, 8, prod))
    head = launch(sr.lower_tf(sub_case(c, 0, cut), 8, prod))
    tail = launch(sr.lower_tf(sub_case(c, cut, B), 8, prod))
    assert torch.equal(whole[:cut], head)
    assert torch.equal(whole[cut:], tail)
    assert not torch.equal(whole[0], whole[1])


def test_zz_dump_ratios():
    """Last in the file: every ratio the run recorded (shown under -s; written to the file that MDT_SPLIT_CORE_RATIOS names).
    A recorder: each case asserts its own ratio."""
    text = json.dumps(RATIOS, indent=0, sort_keys=True)
    print("\n" + text)
    if os.environ.get("MDT_SPLIT_CORE_RATIOS"):
        with open(os.environ["MDT_SPLIT_CORE_RATIOS"], "w") as f:
            f.write(text)
