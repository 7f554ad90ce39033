"""CPU: the references of tests/bf16_ref.py before any GPU run.

(a) every case of tests/test_gpu_bf16_elementwise.py through oracle/program_interp.py, one op per program, under the same criterion:
    this proves the closed forms, the lowering and the per-op chaining;
(b) the criterion discriminates: planted results -- a truncating bf16 store, a small element moved by two of its own ulps, a GELU
    whose erf is off by 1e-4, a one-pass variance accumulated in bf16, a bf16 copy that rounds ties away from zero -- are rejected
    on the new cases, and for each it is recorded whether the present assertion of the corresponding tests/test_gpu_ops.py test
    accepts it on that test's present inputs (the truncating store is accepted there: the reason for this file);
(c) delta <= 1e-4 max(1, |r|max) for every case: the references alone agree."""
import math

import pytest
import torch

import bf16_ref as br
from bf16_ref import BF16, F32
from gpu_util import rnd
from moleculediffusiontransformer_amd import runtime as rt
from oracle.program_interp import Buffers, run_program

CASES = br.all_cases()
IDS = [br.case_id(fn, args) for fn, args in CASES]


def interp(ops, weights, act, shr, B):
    bufs = Buffers(weights.clone(), act, shr.clone(), {})
    run_program(ops, bufs, B, 0)
    return bufs.act


def test_the_list_names_every_site_once():
    assert len(set(IDS)) == len(IDS)
    keys = [br.build(fn, args).key for fn, args in CASES]
    assert len(set(keys)) == len(keys)                                   # (the keys name the ratios of the dump)


@pytest.mark.parametrize("fn,args", CASES, ids=IDS)
def test_interpreter_meets_the_criterion_and_the_references_agree(fn, args):
    c = br.build(fn, args)
    snaps = br.stepwise(c, interp)
    for k in c.check:                                                    # (c)
        for out in br.reference(c, k, snaps[k]):
            assert br.cap_holds(out), (out.name, br.delta(out.r, out.i), out.r.abs().max().item())
    ratios = br.verify(c, snaps)                                         # (a)
    assert ratios and max(ratios.values()) <= 1.0


def test_rne_bits_is_round_to_nearest_even():
    t = br.tie_values()
    got = br.rne_bits(t)
    assert torch.equal(got, br.bits16(t.to(BF16)))                       # torch's conversion agrees on every planted value
    u = t.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    tie = (u & 0xFFFF) == 0x8000
    assert int(tie.sum()) >= 40
    assert bool(((got[tie] & 1) == 0).all())                             # a tie goes to the even neighbour ...
    lower_odd = ((u[tie] >> 16) & 1) == 1
    assert bool(lower_odd.any()) and bool((~lower_odd).any())            # ... from both parities of the lower one
    assert bool((got[tie][lower_odd] == (u[tie][lower_odd] >> 16) + 1).all()) and bool((got[tie][~lower_odd] == u[tie][~lower_odd] >> 16).all())
    big = torch.tensor([0x7F7F7FFF], dtype=torch.int32).view(F32)
    assert br.rne_bits(big).item() == 0x7F7F and br.rne_bits(torch.tensor([-0.0])).item() == 0x8000


def test_cases_that_copy_plant_ties_zeros_and_the_largest_finite_value():
    c = br.build(br.prep16_case, (5, 32, 64, "copy"))
    src = c.act[: 5 * 32 * 64].view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    assert int(((src & 0xFFFF) == 0x8000).sum()) >= 60
    for pattern in (0x00000000, 0x80000000, 0x7F7F7FFF, 0xFF7F7FFF):
        assert bool((src == pattern).any())


# ---- (b) planted faults --------------------------------------------------------------------------------------------------------

def trunc16(x):
    """A bf16 store that drops the low 16 bits of the fp32 value instead of rounding."""
    return (x.float().contiguous().view(torch.int32) & -65536).view(F32).view(x.shape)      # (-65536 = 0xffff0000)


def away16(x):
    """A bf16 conversion that rounds to nearest with ties AWAY from zero."""
    u = x.float().contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    v = ((u + 0x8000) >> 16) << 16
    return (v - ((v >> 31) << 32)).to(torch.int32).view(F32).view(x.shape)


def _gelu_off(x, d):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)) + d)


def _new_case_out(fn, args, k):
    """Output 0 of op k of a new case with the arena in front of it as the interpreter leaves it."""
    c = br.build(fn, args)
    snaps = br.stepwise(c, interp)
    return c, snaps, br.reference(c, k, snaps[k])


def _rejects(G, out):
    try:
        br.check(G, out)
    except AssertionError:
        return True
    return False


def _plant_truncating_store():
    """new: the WFMT 38 op of the residual-stream chain.  old: test_bf16_residual_stream_ops' assertions on (130, 4, 64)."""
    res = {}
    for shape in ((130, 4, 64), (5, 32, 512)):
        c, snaps, outs = _new_case_out(br.chain_case, shape + (-1, 1), 2)
        out = outs[0]
        G = trunc16(out.r.float())
        share = (br.excess(G, out, br.delta(out.r, out.i)) > 1).double().mean().item()
        res[shape] = (_rejects(G, out), share, br.ratio(G, out), br.ratio(out.r.float().to(BF16).float(), out))
    # the present assertions, on the present inputs: out_c from the interpreter, out_g the truncated store of the same sums
    B, R, C = 130, 4, 64
    c, snaps, outs = _new_case_out(br.chain_case, (B, R, C, -1, 1), 2)
    out_c = snaps[3].view(BF16)[outs[0].idx].float()
    out_g = trunc16(outs[0].r.float())
    ok_ulp = (out_g - out_c).abs().max() <= 2.0 ** -6 * max(out_c.abs().max().item(), 1.0)
    want = outs[0].r.float().to(BF16).float()                            # (the closed form of that test: the same three ops)
    ok_closed = (out_g - want).abs().max() <= 2.0 ** -5 * max(want.abs().max().item(), 1.0)
    return res, bool(ok_ulp and ok_closed)


def _plant_two_ulps_on_a_small_element():
    """new: WFMT 6 + GELU.  old: test_gemm_bf16_chain_with_bf16_intermediate's assertion on the hidden tensor (2^-7 of its scale)."""
    c, snaps, outs = _new_case_out(br.b16_case, (5, 32, 64, 96, 3, 6, 1, -1, 1), 0)
    out = outs[0]
    G = out.r.float().to(BF16).float()
    small = ((out.r.abs() > 2e-2) & (out.r.abs() < 6e-2)).nonzero().view(-1)      # (two ulps there: 1.2e-4 to 4.9e-4, several delta)
    assert small.numel() > 0
    k = small[0]
    G2 = G.clone()
    G2[k] = G[k] + 2 * br.ulp_bf16(out.r[k]).float()
    old_ok = (G2 - G).abs().max() <= 2.0 ** -7 * max(G.abs().max().item(), 1.0)
    return _rejects(G2, out), not _rejects(G, out), bool(old_ok)


def _plant_gelu_erf_off():
    """new: WFMT 6 + GELU with erf + 1e-4.  old: the same assertion on the hidden tensor."""
    c, snaps, outs = _new_case_out(br.b16_case, (3, 128, 256, 256, 1, 6, 1, -1, 1), 0)
    out = outs[0]
    op = c.ops[0]
    i = op.i
    a = br._a_rows(c, snaps[0], op, True).double()
    w = br._wide16(br._view(c, snaps[0], op.w, i[rt.G_N] * i[rt.G_CIN] // 2)).view(i[rt.G_N], i[rt.G_CIN]).double()
    pre = a @ w.T + br._view(c, snaps[0], op.bias, i[rt.G_N]).double()
    assert (br._gelu(pre).reshape(-1) - out.r).abs().max() < 1e-12       # (this IS the case's r)
    G = _gelu_off(pre, 1e-4).reshape(-1).float().to(BF16).float()
    good = out.r.float().to(BF16).float()
    old_ok = (G - good).abs().max() <= 2.0 ** -7 * max(good.abs().max().item(), 1.0)
    return _rejects(G, out), bool(old_ok)


def _plant_bf16_variance():
    """new: WFMT 134 with the one-pass sums q and s accumulated in bf16.  old: test_layernorm_folded_into_bf16_gemm's assertions
    (2^-6 of the scale against the interpreter, 3e-2 of it against the closed form) on (67, 2, 64, 128)."""
    res = {}
    for family in br.FOLD_FAMILIES:
        c, snaps, outs = _new_case_out(br.fold_case, (67, 2, 64, 128, family, -1), 0)
        out, op = outs[0], c.ops[0]
        i = op.i
        n, cin = i[rt.G_N], i[rt.G_CIN]
        a = br._a_rows(c, snaps[0], op, True)
        w = br._wide16(br._view(c, snaps[0], op.w, n * cin // 2)).view(n, cin)
        s = torch.zeros(a.shape[:2], dtype=BF16)
        q = torch.zeros(a.shape[:2], dtype=BF16)
        for k in range(cin):
            s = (s.float() + a[:, :, k]).to(BF16)
            q = (q.float() + a[:, :, k] * a[:, :, k]).to(BF16)
        mean = (s.float() / cin).unsqueeze(-1)
        var = (q.float().unsqueeze(-1) / cin - mean * mean).clamp(min=0.0)
        G = ((1.0 / torch.sqrt(var + 1e-5)) * (a @ w.T - mean * br._view(c, snaps[0], op.p0, n)) + br._view(c, snaps[0], op.bias, n))
        G = G.reshape(-1).to(BF16).float()
        good = snaps[1].view(BF16)[out.idx].float()
        scale = max(good.abs().max().item(), 1.0)
        old_ok = (G - good).abs().max() <= 2.0 ** -6 * scale and (G.double() - out.r).abs().max() <= 3e-2 * scale
        res[family] = (_rejects(G, out), bool(old_ok))
    return res


def _plant_ties_away():
    """new: the copy of MDT_OP_PREP16 without prologue.  old: test_gn_act_on_two_sources_with_raw_copy's torch.equal on ITS inputs
    (random fp32 values: no ties among them)."""
    c, snaps, outs = _new_case_out(br.prep16_case, (5, 32, 64, "copy"), 0)
    out = outs[0]
    src = c.act[: 5 * 32 * 64]
    G = away16(src).to(BF16)
    B, R, C = 3, 4, 64
    xa, xb = rnd(B * R * C, seed=4) * 1.5 + 0.3, rnd(B * R * C, seed=5) * 0.8 - 0.2
    cat = torch.cat([xa.view(B, R, C), 0.7071 * xb.view(B, R, C)], dim=2)
    old_ok = torch.equal(away16(cat).to(BF16), cat.to(BF16))
    return _rejects(G, out), not _rejects(src.to(BF16), out), bool(old_ok)


def test_planted_faults_are_rejected_and_the_old_assertions_miss_the_truncating_store():
    table = {}
    res, old = _plant_truncating_store()
    for shape, (rejected, share, bad, good) in res.items():
        assert rejected and share > 0.3 and bad > 100 and good <= 1.0, (shape, rejected, share, bad, good)
    assert old, "the present assertions of test_bf16_residual_stream_ops were expected to accept a truncating store"
    table["truncating bf16 store (WFMT 38)"] = dict(new="rejected", old="accepted", share=[round(v[1], 3) for v in res.values()],
                                                    ratio=[round(v[2], 1) for v in res.values()], rounded=[round(v[3], 4) for v in res.values()])
    rejected, clean_ok, old = _plant_two_ulps_on_a_small_element()
    assert rejected and clean_ok
    table["small element moved by 2 of its ulps (WFMT 6)"] = dict(new="rejected", old="accepted" if old else "rejected")
    rejected, old = _plant_gelu_erf_off()
    assert rejected
    table["GELU with erf + 1e-4 (WFMT 6)"] = dict(new="rejected", old="accepted" if old else "rejected")
    for family, (rejected, old) in _plant_bf16_variance().items():
        assert rejected, family
        # (the present test has the mean-0.7 rows only)
        table[f"one-pass variance in bf16 (WFMT 134, {family})"] = dict(new="rejected", old=("accepted" if old else "rejected") if family == "mean 0.7" else "no such input")
    rejected, clean_ok, old = _plant_ties_away()
    assert rejected and clean_ok
    table["bf16 copy, ties away from zero"] = dict(new="rejected", old="accepted" if old else "rejected")
    import json
    print("\n" + json.dumps(table, indent=1))                            # (shown under -s: the table of DESIGN.md 4.3)
