"""CPU: tests/norm_ref.py is a fit yardstick for tests/test_gpu_norm_range.py -- no budget is loose (the cap holds
for every case the GPU test runs), the CPU interpreter and the correct fp32 form meet the criterion on every case, every eps a
kernel takes moves some case's R by more than ten budgets, the planted faults are rejected on their families, and the table says
which of them the present assertions of tests/test_gpu_ops.py accept on that file's present inputs."""
import collections

import pytest
import torch

import norm_ref as nr
from moleculediffusiontransformer_amd import runtime as rt
from norm_ref import CASES, F32, PRESENT, build, case_id
from oracle.program_interp import Buffers, run_program


def interp(lowered):
    ops, weights, act, shr, ext, B, out = lowered[:7]
    bufs = Buffers(weights.clone(), act.clone(), shr.clone(), {k: v.clone().view(-1) for k, v in ext.items()})
    run_program(ops, bufs, B, 0)
    return out(bufs.act)


def rejected(G, refs, split):
    try:
        nr.check(G, refs, split)
    except AssertionError:
        return True
    return False


def widest(c):
    """The wider of the budgets a case is held to: a fault rejected under it is rejected in both product modes."""
    return c.ring or c.split


# ---- 1. the cap, the interpreter, the correct fp32 form ----------------------------------------------------------------------------

@pytest.mark.parametrize("entry", CASES, ids=case_id)
def test_cap_holds_and_the_interpreter_meets_the_criterion(entry):
    """Every (site, shape, family, eps) x product mode of the GPU test: 8 e_ref (+ 4 e16) <= 5e-3 max(1, |R|max), so the case runs
    and says something; the interpreter -- what run_both returns beside the GPU's result -- and I itself are within the budget."""
    c = build(entry)
    for prod in c.prods():
        split = c.is_split(prod)
        assert nr.cap_holds(c.refs, split), (case_id(entry), prod, c.refs.e_ref, c.refs.e16)
        lowered = c.lower(prod)
        assert sum(lowered[8]) * lowered[5] == lowered[2].numel(), "the arena is its tensors, one after the other"
        nr.check(interp(lowered), c.refs, split)
        assert not rejected(c.refs.I, c.refs, split)


def test_every_family_is_what_it_claims():
    """Row statistics of the LayerNorm input and (sample, group) statistics of the GroupNorm input, as DESIGN.md 4.4 states them."""
    x = {f: nr.ln_input(f, 37, 4096) for f in nr.FAMILIES}
    m, s = {f: v.double().mean(1) for f, v in x.items()}, {f: v.double().std(1) for f, v in x.items()}
    assert (m["unit"] - 0.3).abs().max() < 0.1 and (s["unit"] - 1.5).abs().max() < 0.1
    assert (m["offset"] - 64).abs().max() < 0.1 and (s["offset"] - 1).abs().max() < 0.1
    assert m["tiny"].abs().max() < 1e-4 and (s["tiny"] * 1024 - 1).abs().max() < 0.1
    assert (s["tiny"] ** 2).max() < 1.1e-6                              # the variance lies under both eps values
    assert torch.equal(x["huge"], x["unit"] * 4096)                     # exactly: a power of two
    cls = nr.ln_classes(37)
    assert cls[-1] == 2 and set(cls.tolist()) == {0, 1, 2, 3}           # the last valid row is an all-zero row
    mx = x["mixed"]
    assert torch.equal(mx[cls == 0], x["unit"][cls == 0] * 4096) and torch.equal(mx[cls == 1], x["unit"][cls == 1] * 2.0 ** -12)
    assert (mx[cls == 2] == 0).all() and torch.equal(mx[cls == 3], x["offset"][cls == 3])
    # GroupNorm: neighbouring groups of a sample differ in class, and so do neighbouring samples at the same group
    g = nr.gn_classes(5, 8)
    assert (g[:, 1:] != g[:, :-1]).all() and (g[1:] != g[:-1]).all()
    xg = nr.gn_input("mixed", 5, 4, 512, 8).view(5, 4, 8, 64)
    for b in range(5):
        for k in range(8):
            u = xg[b, :, k]
            want = {0: 1.5 * 4096, 1: 1.5 * 2.0 ** -12, 2: 0.0, 3: 1.0}[int(g[b, k])]
            assert abs(u.double().std().item() - want) <= 0.15 * want


# ---- 2. every eps of every kernel matters somewhere ----------------------------------------------------------------------------------

def test_every_eps_of_every_kernel_moves_some_case_by_ten_budgets():
    """eps_ln, eps_gn, eps_res of the whole-level kernels and the single eps of the others: replaced ALONE by the other model value
    (1e-5 <-> 1e-6), in fp64, it moves R of at least one case of that kernel by more than 10 budgets (the wider budget).  This is
    what a swap of two eps values in mdt_api.cpp or in the compiler would be caught by."""
    best = collections.defaultdict(float)
    for entry in CASES:
        c = build(entry)
        if c.family not in ("tiny", "tiny_ln", "tiny_mid"):
            continue
        bud = nr.budget(c.refs, widest(c))
        for name in c.eps:
            best[(c.kernel, name)] = max(best[(c.kernel, name)], c.eps_shift(name) / bud)
    want = {(build(e).kernel, name) for e in CASES for name in build(e).eps}
    assert want == set(best), want ^ set(best)
    print()
    for k, v in sorted(best.items()):
        print(f"{k[0]} {k[1]}: R moves by {v:.3g} budgets")
        assert v > 10, k
    assert {k for k, _ in best} >= {"k_tf128", "k_tf256", "k_res256", "k_rconv", "k_proj", "k_resblock", "k_gn_act", "k_gn_stats<64>",
                                   "k_gn_stats<256>", "k_gemm LN", "k_gemm GN", "k_gemm_bf16x3", "k_gemm_as", "k_tblock_lw", "k_tblock32"}
    assert {n for k, n in best if k == "k_tf128"} == {"eps_ln", "eps_gn", "eps_res"}


# ---- 3. planted faults in the fp32 form ---------------------------------------------------------------------------------------------

RES_SITES = ("k_resblock GN", "k_tf128 ResNet GN", "k_res256 GN")
TINY = ("tiny", "tiny_ln", "tiny_mid")


def fault_applies(fault, c):
    """Is `fault` something this case can see at all?  (Not: is it rejected.)"""
    if c.site == "k_gn_stats mean" and fault in ("onepass", "eps_swap", "std_eps"):
        return False                                     # the mean does not depend on the variance or on eps
    if fault == "onepass":
        # a ResNet block adds a convolution of its RAW input: at `offset` that term sets |R|max (120 - 180) and e16, and the budget
        # with them -- its GroupNorms are held to the one-pass variance on offset_mid instead
        return c.family == ("offset_mid" if c.site in RES_SITES else "offset")
    if fault in ("eps_swap", "std_eps"):
        return c.family in TINY
    if c.family != "mixed":
        return False
    if fault == "pooled":
        return not (c.site == "k_resblock GN" and c.shape[2] == 1)      # (B = 1 with one group: the unit has no neighbour)
    return c.pad_rows > 0 and c.rows > 1                 # clamped: duplicates of a unit's ONLY row leave its statistics as they are


@pytest.mark.parametrize("fault", nr.FAULTS)
def test_planted_fault_is_rejected_on_its_family(fault):
    """one-pass variance on offset; swapped eps and 1 / (std + eps) on tiny; statistics pooled over two neighbouring units, and
    taken over the clamped duplicate rows of a partial tile, on mixed: the kernel's fp32 form with that one fault is outside the
    (wider) budget on EVERY case of the family that can see it, at every site."""
    seen = collections.Counter()
    for entry in CASES:
        c = build(entry)
        if not fault_applies(fault, c):
            continue
        r = nr.ratio(c.eval(F32, fault=fault), c.refs, widest(c))
        assert r > 1.0, (fault, case_id(entry), r)
        seen[c.site] += 1
    print(f"\n{fault}: rejected on {sum(seen.values())} cases at {len(seen)} sites: {dict(seen)}")
    sites = {build(e).site for e in CASES}
    if fault == "clamped":
        assert set(seen) == {"k_rconv GN", "k_rconv GN, two sources", "k_tf128 ResNet GN", "k_res256 GN", "k_tf128 LN, to_in GN",
                             "k_tf256 LN, to_in GN"}
    elif fault == "pooled":
        assert set(seen) == sites
    else:
        assert set(seen) == sites - {"k_gn_stats mean"}


# ---- 4. what the present assertions see ----------------------------------------------------------------------------------------------

def _old(site, shape, prod, tol_interp, tol_form, relative):
    return dict(site=site, shape=shape, prod=prod, tol_interp=tol_interp, tol_form=tol_form, relative=relative)


GN, LN = rt.PRO_GROUPNORM, rt.PRO_LAYERNORM
# the assertion of the corresponding tests/test_gpu_ops.py test: |G - interpreter| < tol_interp, |G - closed form| < tol_form
# (None: the test has no closed form), both times max(1, |interpreter|max) where `relative`
OLD = [
    _old(nr.gemm_ln_case, (3, 12, 128, 1024), None, 3e-5, 3e-5, False),               # test_gemm_layernorm_prologue
    _old(nr.gemm_gn_case, (5, 4, 512, 8), None, 5e-5, 5e-5, False),                   # test_gn_stats_and_groupnorm_prologue
    _old(nr.gemm_gn_case, (2, 32, 32, 32), None, 5e-5, 5e-5, False),
    _old(nr.split_gemm_case, (3, 16, 128, 96, 3), None, 4e-5, None, True),            # test_gemm_split_bf16
    _old(nr.split_gemm_case, (40, 4, 256, 256, 1), None, 4e-5, None, True),
    _old(nr.gn_act_case, (3, 16, 128, 8, True, True, 1e-5), None, 2e-5, 2e-5, False),  # test_gn_act
    _old(nr.gn_act_case, (2, 4, 256, 32, False, False, 1e-6), None, 2e-5, 2e-5, False),
    _old(nr.proj_case, (37, 1, 256, 1024, "affine", False), "f32", 1e-5, 1e-5, False),  # test_row_stationary_projection_on_ring_tiles
    _old(nr.proj_case, (5, 4, 128, 64, "plain", True), "f32", 1e-5, 1e-5, False),
    _old(nr.rconv_case, (128, 16, 5, 3, 16, True, True, "other", 1.0), "f32", 1e-4, 1e-4, True),   # test_row_stationary_conv
    _old(nr.rconv_case, (256, 4, 9, 3, 64, False, True, "accumulate", 0.7071), "f32", 1e-4, 1e-4, True),
]
# fault -> the sites of OLD whose present assertion REJECTS it on the present inputs ("all": every one that can show the fault).
# The exact-product k_proj test holds 1e-5, close enough to see an eps of 1e-6 for 1e-5 at std 1.3 (the split-bf16 run of the same
# test holds 5e-5 / 1e-4); test_gn_act's 2e-5 sees 1 / (std + eps) where FiLM and SiLU follow.  Everything else passes.
OLD_REJECTS = {"onepass": set(), "eps_swap": {"k_proj LN"}, "std_eps": {"k_proj LN", "k_gn_act (3, 16, 128, 8, True, True)"},
               "pooled": "all", "clamped": "all"}


def old_accepts(G, interp_out, R, o):
    scale = max(1.0, interp_out.abs().max().item()) if o["relative"] else 1.0
    ok = (G - interp_out).abs().max().item() < o["tol_interp"] * scale
    if o["tol_form"] is not None:
        ok = ok and (G.double() - R).abs().max().item() < o["tol_form"] * scale
    return ok


@pytest.mark.parametrize("fault", nr.FAULTS)
def test_what_the_present_assertions_accept(fault):
    """The "old assertion" column of DESIGN.md 4.4: the faulty fp32 form on the inputs tests/test_gpu_ops.py has always used (mean
    0.2 - 0.5, std 1.3 - 2), judged as that file judges a GPU result.  The three faults of the arithmetic pass it nearly everywhere
    (OLD_REJECTS) -- which is why the suite could not see them; pooled and clamped statistics are order-1 errors on any input and are
    rejected there too (what the new inputs add for them is the contrast in SCALE between neighbours: the all-zero row, 2^24
    between two units)."""
    verdicts = []
    for o in OLD:
        fn = o["site"]
        eps = o["shape"][6] if fn is nr.gn_act_case else nr.GN_PROD_EPS[o["shape"]] if fn is nr.gemm_gn_case else 1e-5
        args = (o["shape"], PRESENT, {"eps": eps})      # (the eps the test_gpu_ops.py tuple runs with)
        if fn is nr.split_gemm_case:
            for pro in (LN, GN):
                verdicts.append((o, fn(*args, pro)))
        else:
            verdicts.append((o, fn(*args)))
    out = []
    for o, c in verdicts:
        if fault == "clamped" and not (c.pad_rows and c.rows > 1):
            continue
        C = interp(c.lower(o["prod"])).reshape(c.refs.R.shape)
        assert old_accepts(c.refs.I, C, c.refs.R, o), (c.key, "the correct form must pass the old assertion")
        out.append((c.key, c.site, f"{c.site} {c.shape}", old_accepts(c.eval(F32, fault=fault), C, c.refs.R, o)))
    print()
    assert out
    for key, site, site_shape, ok in out:
        print(f"{fault}: old assertion {'ACCEPTS' if ok else 'rejects'} on {key}")
        want_reject = OLD_REJECTS[fault] == "all" or site in OLD_REJECTS[fault] or site_shape in OLD_REJECTS[fault]
        assert ok != want_reject, (fault, key, ok)
