"""-m gpu: every place the plain-bf16 mode (gemm_mode = 'bf16') rounds, element by element, against the fp64 closed forms of
tests/bf16_ref.py -- the criterion is stated once, in that module's docstring (DESIGN.md 4.3 holds the table of ratios).

  site                                 ops / formats                                               cases (bf16_ref.all_cases)
  -----------------------------------  ----------------------------------------------------------  --------------------------------
  k_prep16, k_prep16_ln_in16           MDT_OP_PREP16: copy (ties planted), LayerNorm, GroupNorm     prep16_case x (5,32,64) (3,128,256)
                                       + FiLM + SiLU after MDT_OP_GN_STATS, SiLU, WFMT 2            (130,4,64)
  k_gemm3 plain-bf16 path              MDT_G_WFMT 1, prologue GroupNorm / none / SiLU, fp32 out     wfmt1_case (3,16,128,96,3) (5,64,32,64,3)
                                       + residual                                                   (33,1,256,160,1)
  k_gemm_b16                           WFMT 2 (taps 3 and 1), 6 (+- GELU; w16 1 / 0), 10 (copy,     b16_case (5,32,64,96,3) (3,128,256,256,1);
                                       ties planted), 38 in place; tile16 -1, 0, 1, 2               single_chunk_case (83,4,64,64); chain_case
                                                                                                    (130,4,64->128->64) (5,32,512->1024->512);
                                                                                                    column_block_case (41,8,256,128) in (320, 64)
  k_gemm_b16, folded LayerNorm         WFMT 134, every tile, rows of mean 0.7 / std 1.5 and of      fold_case (67,2,64,128) (130,4,256,768);
                                       mean 4 / std 0.5; the column-block form                      column_block_case(fold)
  k_gn_act                             bf16 output on every dispatch branch of launch_gn_act;       gn_act_case x 10, gn_two_case (3,4,64,4)
                                       two sources + raw copy (ties planted)                        (37,8,1024,8)

Left out because the ABI refuses them: WFMT 134 with w16 = 0 ("a folded LayerNorm lives in the all-bf16 epilogue only": the switch is
ignored for it, k_gemm_b16.hip gemm_b16_w16_ok), so the fold runs with the tile switch alone.  The bf16-operand attention cores are
tests/test_gpu_softmax_range.py's.

Every op runs as a program of its own on the arena the previous one left (bf16_ref.stepwise): r comes from the GPU's own bits.
Every case records ratio = max((|G - r| - ulp / 2) / delta); the last test dumps them.  A ratio above 1 is a finding in the kernel,
not a reason to touch a margin."""
import json
import os

import pytest
import torch

import bf16_ref as br
from gpu_util import DEV
from moleculediffusiontransformer_amd import runtime as rt

pytestmark = pytest.mark.gpu

CASES = br.all_cases()
RATIOS = {}


def gpu(ops, weights, act, shr, B):
    gw, ga, gs = weights.to(DEV), act.to(DEV), shr.to(DEV)
    b = rt.MdtBindings()
    b.weights, b.act, b.shr = rt.ptr(gw), rt.ptr(ga), rt.ptr(gs)
    with torch.cuda.device(DEV):
        rt.Program(ops).run(b, B, 0)
        torch.cuda.synchronize()
    return ga.cpu()


def record(G, out):
    """check() with the figures kept first: a failing case still shows its ratio in the dump."""
    if out.kind != "copy":
        d = br.delta(out.r, out.i)
        r = br.ratio(G, out)
        RATIOS[out.name] = dict(ratio=round(r, 4), delta=d, rmax=round(out.r.abs().max().item(), 3), kind=out.kind)
        print(f"\n{out.name}: {out.kind} delta {d:.3g} |r|max {out.r.abs().max().item():.3g} ratio {r:.4f}")
    else:
        RATIOS[out.name] = dict(kind="copy", elements=int(out.bits.numel()))
    return br.check(G, out)


@pytest.mark.parametrize("fn,args", CASES, ids=[br.case_id(fn, args) for fn, args in CASES])
def test_bf16_mode_element_by_element(fn, args):
    c = br.build(fn, args)
    lib = rt.load_library()
    if c.tile is not None:
        lib.mdt_set_tuning(b"tile16", int(c.tile))
    if c.w16 is not None:
        lib.mdt_set_tuning(b"w16", int(c.w16))
    try:
        snaps = br.stepwise(c, gpu)
    finally:
        lib.mdt_set_tuning(b"tile16", -1)
        lib.mdt_set_tuning(b"w16", 1)
    ratios = br.verify(c, snaps, judge=record)
    assert ratios and max(ratios.values()) <= 1.0


def test_zz_dump_ratios():
    """Last in the file: every ratio the run recorded, as one JSON object (shown under -s; written to the file that
    MDT_BF16_RATIOS names), and the largest per site.  A recorder: each case asserts its own ratio."""
    text = json.dumps(RATIOS, indent=0, sort_keys=True)
    print("\n" + text)
    if os.environ.get("MDT_BF16_RATIOS"):
        with open(os.environ["MDT_BF16_RATIOS"], "w") as f:
            f.write(text)
    sites = {}
    for fn, args in CASES:
        c = br.build(fn, args)
        for name, v in RATIOS.items():
            if name.startswith(c.key + " op ") and "ratio" in v:
                if v["ratio"] > sites.get(c.site, (-1.0, ""))[0]:
                    sites[c.site] = (v["ratio"], name)
    for site, (r, name) in sorted(sites.items()):
        print(f"largest ratio, {site}: {r:.4f} at {name}")
