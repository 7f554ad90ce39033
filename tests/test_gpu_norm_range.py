"""-m gpu: every hand-written LayerNorm / GroupNorm section of csrc/ in the default (bf16x3) and exact (f32) modes -- k_gn_stats,
the GEMM prologues (k_gemm, k_gemm_bf16x3, k_gemm_as), k_gn_act, k_proj, k_rconv, k_resblock, k_tblock_lw, k_tblock32 and the norms
inside k_tf128, k_tf256, k_res256 -- on rows that leave mean 0.3 / std 1.5: offset (mean 64), tiny (std 2^-10: the variance lies
under eps), huge (times 2^12), mixed (neighbouring units 2^24 apart in scale, all-zero units), at the site's eps and at the other
model value, against the fp64 closed forms of tests/norm_ref.py.  DESIGN.md section 4.4.

The budget is softmax_ref.check()'s: 8 e_ref (+ 4 e16 on a split-bf16 path) + 2e-6 max(1, |R|max), e_ref and e16 measured between
references.  Every case records max|G - R| / budget; the last test of the file dumps them.  A ratio above 1 is a finding in the
kernel, not a reason to touch a margin."""
import json
import os

import pytest
import torch

import norm_ref as nr
from gpu_util import DEV, run_both
from norm_ref import CASES, build, case_id
from poison_util import gpu_run
from test_gpu_ops import prod      # noqa: F401  (fixture: split-bf16 / exact-fp32 ring tiles)

pytestmark = pytest.mark.gpu

RATIOS = {}
RING = [e for e in CASES if e[0] in (nr.proj_case, nr.rconv_case, nr.rconv2_case, nr.resblock_case, nr.tblock_case, nr.tf_case,
                                     nr.res128_case, nr.res256_case)]
PLAIN = [e for e in CASES if e not in RING]


def launch_gpu(lowered):
    """The program on the GPU alone, from fresh copies of its buffers: (act, weights, shr, ext) as the launch left them."""
    ops, weights, act, shr, ext, B = lowered[:6]
    gw, ga, gs = weights.to(DEV), act.to(DEV), shr.to(DEV)
    ge = {k: v.to(DEV).contiguous() for k, v in ext.items()}
    gpu_run(ops, gw, ga, gs, ge, B)
    return ga.cpu(), gw.cpu(), gs.cpu(), {k: v.cpu() for k, v in ge.items()}


def run(c, prod_):
    """One case in one product mode: through run_both (GPU and interpreter), then the same launch again.  Returns the GPU's result in
    the shape of R.  Asserts what every case asserts beside its budget: finite, inputs / weights / shared rows bit for bit, the
    second launch bit for bit, no hand-off poll timed out, and the interpreter within the same budget."""
    lowered = c.lower(prod_)
    ops, weights, act, shr, ext, B, out, untouched = lowered[:8]
    (ga, gs, ge), (ca, _, _) = run_both(ops, weights, act, shr, ext, B)
    for lo, hi in untouched:
        assert torch.equal(ga[lo:hi], act[lo:hi]), "an input was written"
    assert torch.equal(gs, shr), "the shared rows were written"
    if 3 in ge:
        assert int(ge[3].view(torch.int32)[0]) == 0, "a hand-off poll timed out"
    ga2, gw2, gs2, _ = launch_gpu(lowered)
    assert torch.equal(ga2.view(torch.int32), ga.view(torch.int32)), "the same launch twice gives other bits"
    assert torch.equal(gw2, weights) and torch.equal(gs2, shr), "weights or shared rows were written"
    G = out(ga).reshape(c.refs.R.shape)
    assert torch.isfinite(G).all()
    split = c.is_split(prod_)
    r = nr.ratio(G, c.refs, split)
    ri = nr.ratio(out(ca).reshape(c.refs.R.shape), c.refs, split)
    mode = prod_ or ("bf16x3" if split else "f32")
    RATIOS[f"{c.key} {mode}"] = dict(site=c.site, kernel=c.kernel, shape=str(c.shape), family=c.family, eps=c.eps, products=mode,
                                     rmax=c.refs.R.abs().max().item(), e_ref=c.refs.e_ref, e16=c.refs.e16,
                                     budget=nr.budget(c.refs, split), ratio=round(r, 4), interpreter=round(ri, 4),
                                     e_ref_subtract_first=c.e_ref_subtract_first if c.gn else None)
    print(f"\n{c.key} {mode}: |R|max {c.refs.R.abs().max():.3g} e_ref {c.refs.e_ref:.3g} e16 {c.refs.e16:.3g} "
          f"budget {nr.budget(c.refs, split):.3g} ratio {r:.3f} (interpreter {ri:.3f})")
    assert nr.cap_holds(c.refs, split)
    nr.check(G, c.refs, split)
    assert ri <= 1.0, "the interpreter misses the budget"
    return G


def zero_units(c, B, G):
    """[B, G] mask of the all-zero (sample, group) units of a `mixed` GroupNorm input."""
    return nr.gn_classes(B, G) == 2


@pytest.mark.parametrize("entry", PLAIN, ids=case_id)
def test_norm_range(entry):
    """MDT_OP_GN_STATS read back from the arena, the prologues of k_gemm / k_gemm_bf16x3 / k_gemm_as, k_gn_act with one and two
    sources (fp32 output)."""
    c = build(entry)
    G = run(c, None)
    if c.family != "mixed":
        return
    fn, args = entry
    if fn is nr.gn_stats_case:
        (B, _, _, groups), what = c.shape, args[3]
        zero = zero_units(c, B, groups)
        assert zero.any()
        if what == "mean":                              # an all-zero unit: mean exactly 0.0f
            assert (G[zero].view(torch.int32) == 0).all()
        else:                                           # ... and rstd within one fp32 ulp of 1 / sqrt(eps)
            want = torch.full_like(G[zero], 1.0, dtype=torch.float64) / torch.tensor(nr.f32(c.eps["eps"]), dtype=torch.float64).sqrt()
            off = ((G[zero].double() - want).abs() / nr.ulp32(want)).max().item()
            print(f"rstd of an all-zero unit: {off:.3f} ulp from 1 / sqrt(eps)")
            assert off <= 1.0
    if fn is nr.gn_act_case and not (c.shape[4] or c.shape[5]):
        # without FiLM and SiLU an all-zero unit returns beta bit for bit: 0 * sc + (beta - sc * 0)
        B, R, C, groups = c.shape[:4]
        zero = zero_units(c, B, groups)
        assert zero.any()
        got = G.view(B, R, groups, C // groups).permute(0, 2, 1, 3)[zero]           # [units, R, gs]
        want = c.beta.view(1, groups, 1, C // groups).expand(B, groups, R, -1)[zero]
        assert torch.equal(got.contiguous().view(torch.int32), want.contiguous().view(torch.int32))


@pytest.mark.parametrize("entry", RING, ids=case_id)
def test_norm_range_ring(entry, prod):
    """The ring kernels, split-bf16 and exact-fp32 tiles: k_proj, k_rconv (one and two sources), k_resblock, k_tblock_lw /
    k_tblock32 (self and cross blocks), k_tf128 / k_tf256 (LayerNorms, to_in's GroupNorm, whole and pair-split) and the ResNet
    GroupNorms inside k_tf128 and k_res256."""
    run(build(entry), prod)


# one shape per ring kernel: (builder, leading arguments, eps); k_proj and k_rconv without a residual operand, which the builders
# draw per batch
ALONE = [(nr.proj_case, ((37, 1, 256, 1024, "affine", False),), {"eps": 1e-5}),
         (nr.rconv_case, ((256, 1, 33, 3, 32, False, True, None, 1.0),), {"eps": 1e-5}),
         (nr.resblock_case, ((2, 16, 7, True),), {"eps": 1e-5}),
         (nr.tblock_case, (("k_tblock_lw", 0, 128, 1, 70), 0), {"eps_ln": 1e-5}),
         (nr.tblock_case, (("k_tblock32", 2, 256, 4, 37), 0), {"eps_ln": 1e-5}),
         (nr.tf_case, (("k_tf128", 128, 2, 33, 1, False, "whole"),), dict(nr.TF_EPS)),
         (nr.tf_case, (("k_tf256", 256, 4, 37, 2, True, "whole"),), dict(nr.TF_EPS)),
         (nr.res128_case, ((1, 4, 18, 2, 1),), dict(nr.RES128_EPS)),
         (nr.res256_case, ((2, 8, 5, 2, "pair8"),), {"eps_res": 1e-5})]


@pytest.mark.parametrize("fn,args,eps", ALONE, ids=[a[0].__name__[:-5] + "-" + str(a[1][0][:4]) for a in ALONE])
def test_mixed_units_do_not_depend_on_their_neighbours(fn, args, eps, prod):
    """In `mixed` the rows of a unit sit beside units 2^24 away in scale and beside all-zero ones.  Every fourth sample -- for the
    kernels with one row per sample: the rows of ONE scale class; otherwise the samples of one phase of the cycle -- run alone, as a
    batch of their own, gives the bits it had in the mixed batch (as test_tf128_core_is_position_invariant does for the cores)."""
    full = fn(*args, "mixed", eps)
    B = full.lower(prod)[5]
    rows = list(range(1, B, 4))
    part = fn(*args, "mixed", eps, B_rows=rows)

    def result(c):
        lowered = c.lower(prod)
        ga = launch_gpu(lowered)[0]
        return lowered[6](ga)
    G, P = result(full), result(part)
    G = G.reshape(B, -1)[rows]
    assert torch.isfinite(P).all()
    differ = int((P.reshape(len(rows), -1).contiguous().view(torch.int32) != G.contiguous().view(torch.int32)).sum())
    assert differ == 0, f"{differ} of {G.numel()} floats differ, by up to {(P.reshape(len(rows), -1) - G).abs().max().item():.3g}"


def test_zz_dump_ratios():
    """Last in the file: every figure the run recorded, as one JSON object (shown under -s; written to the file that
    MDT_NORM_RATIOS names), and the largest ratio per product mode.  A recorder: each case asserts its own ratio."""
    text = json.dumps(RATIOS, indent=0, sort_keys=True)
    print("\n" + text)
    if os.environ.get("MDT_NORM_RATIOS"):
        with open(os.environ["MDT_NORM_RATIOS"], "w") as f:
            f.write(text)
    for mode in ("f32", "bf16x3"):
        rs = [v["ratio"] for v in RATIOS.values() if v["products"] == mode]
        if rs:
            print(f"largest ratio, {mode}: {max(rs):.3f} over {len(rs)} cases")
