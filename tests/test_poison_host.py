"""CPU half of the poisoning tests: the harness discriminates -- planted out-of-footprint reads and writes are
rejected under NaN / garbage and invisible under zeros, which is all the suite's inputs ever held -- and the compiled programs,
run through the interpreter, do not depend on what the activation arena (and the per-row FiLM table) holds at the start."""
import functools

import pytest
import torch

from conftest import load_golden
from gpu_util import ref, rnd
from moleculediffusiontransformer_amd import runtime as rt
from moleculediffusiontransformer_amd.compiler import EXT_CTX, EXT_FILM, EXT_OUT, EXT_XIN, compile_unet
from moleculediffusiontransformer_amd.synth import make_synth_model
from oracle.program_interp import Buffers, run_program
from poison_util import (GARBAGE, GUARD, NAN, NAN_BITS, ZERO, TracingBuffers, check_poisoned, fill_bits, fill_floats, interp_run,
                         trace_program)

W, A = rt.SP_WEIGHT, rt.SP_ACT


# ---------------------------------------------------------------------------------------------------------------- fills
def test_fills_are_what_they_claim():
    nan = fill_bits(NAN, 8)
    assert int(nan[0]) == NAN_BITS and torch.isnan(nan.view(torch.float32)).all() and torch.isnan(nan.view(torch.bfloat16).float()).all()
    assert not torch.isnan(torch.tensor([0x7FC00000], dtype=torch.int32).view(torch.bfloat16).float()).all()     # why not the plain NaN
    g = fill_bits(GARBAGE, 4096, seed=3)
    assert torch.equal(g, fill_bits(GARBAGE, 4096, seed=3)) and not torch.equal(g, fill_bits(GARBAGE, 4096, seed=4))
    for v in (g.view(torch.float32), g.view(torch.bfloat16).float()):
        assert torch.isfinite(v).all() and v.abs().min() >= 990.0 and v.abs().max() <= 10100.0
        assert 0.3 < (v > 0).float().mean() < 0.7
    assert int(fill_bits(ZERO, 5).abs().max()) == 0 and GUARD == 64 * 1024


# -------------------------------------------------------------------------------------------------------------- tracing
def _gemm(B=3, R=5, cin=12, lda=16, N=8, gap=2 * 16):
    """One plain OP_GEMM: A rows of `cin` live columns at pitch `lda` (padding columns inside the rows), then `gap` floats nobody
    owns (zeros, as the suite's arenas have), then the output.  Returns ops, weights, act and the extents."""
    op = rt.MdtOp()
    op.kind = rt.OP_GEMM
    a_floats = R * lda
    op.a, op.w, op.bias, op.out = ref(A, 0), ref(W, 0), ref(W, N * cin), ref(A, a_floats + gap)
    i = op.i
    i[rt.G_R_OUT], i[rt.G_R_IN], i[rt.G_LDA], i[rt.G_CIN], i[rt.G_TAPS], i[rt.G_T_STRIDE], i[rt.G_O_STRIDE] = R, R, lda, cin, 1, 1, 1
    i[rt.G_N], i[rt.G_LDC], i[rt.G_O_ROWS] = N, N, R
    weights = torch.cat([rnd(N * cin, seed=1), rnd(N, seed=2), torch.zeros(7)])      # 7 floats behind the bias: nobody's
    act = torch.zeros(B * (a_floats + gap + R * N) + 5)                              # 5 floats behind the output: nobody's
    act[: B * a_floats] = rnd(B * a_floats, seed=3)
    return [op], weights, act, dict(B=B, R=R, cin=cin, lda=lda, N=N, gap=gap, a=B * a_floats, out=B * (a_floats + gap))


def test_footprint_of_a_gemm_is_its_operands_extents():
    ops, weights, act, d = _gemm()
    tb = TracingBuffers(weights.clone(), act.clone(), torch.zeros(4), {})
    trace_program(ops, tb, d["B"])
    own_a, own_w = tb.owned("act"), tb.owned("weights")
    B, R, N = d["B"], d["R"], d["N"]
    # the A rows whole, padding columns up to lda INSIDE (the act offset scaled by B); what lies behind the last row is outside
    assert own_a[: d["a"]].all() and not own_a[d["a"]: d["out"]].any()
    assert own_a[d["out"]: d["out"] + B * R * N].all() and not own_a[d["out"] + B * R * N:].any()
    assert int(own_a.sum()) == d["a"] + B * R * N
    assert own_w[: N * d["cin"] + N].all() and not own_w[N * d["cin"] + N:].any()
    assert not tb.owned("shr").any()
    assert tb.ops_at("act", 0) == [0] and tb.ops_at("act", d["a"]) == []


# -------------------------------------------------------------------------------------------------- the harness discriminates
def _shifted_read(ops, weights, act, shr, ext, B, n_shr=0):
    """Planted: the A operand one row late -- its last row comes from the floats behind the operand."""
    i = ops[0].i
    lda, a_n = i[rt.G_LDA], B * i[rt.G_R_IN] * i[rt.G_LDA]
    scratch = act.clone()
    scratch[:a_n] = act[lda: lda + a_n]               # what a pointer advanced by one row sees
    run_program(ops, Buffers(weights, scratch, shr, ext), B, n_shr)
    o, n = ops[0].out.off * B, B * i[rt.G_O_ROWS] * i[rt.G_LDC]
    act[o: o + n] = scratch[o: o + n]


def _zero_times_garbage(ops, weights, act, shr, ext, B, n_shr=0):
    """Planted: 0 * (a float nobody owns) added to the output -- a multiplication where a select belongs."""
    interp_run(ops, weights, act, shr, ext, B, n_shr)
    o = ops[0].out.off * B
    act[o] += 0.0 * act[o - 1]


def _store_behind_output(ops, weights, act, shr, ext, B, n_shr=0):
    """Planted: a ragged last tile that stores one float too many (a zero)."""
    interp_run(ops, weights, act, shr, ext, B, n_shr)
    o = ops[0].out.off * B + B * ops[0].i[rt.G_O_ROWS] * ops[0].i[rt.G_LDC]
    act[o] = 0.0


def _fmax_with_neighbour(ops, weights, act, shr, ext, B, n_shr=0):
    """Planted: fmaxf against a float nobody owns -- a NaN there is swallowed, a large finite value is not."""
    interp_run(ops, weights, act, shr, ext, B, n_shr)
    o = ops[0].out.off * B
    act[o] = torch.fmax(act[o], act[o - 1].abs() - 1.0e5 * (act[o - 1] == 0))      # (under zeros: max(y, -1e5) = y)


def test_honest_runner_passes_and_returns_what_run_both_returns():
    ops, weights, act, d = _gemm()
    (ga, gs, ge), (ca, cs, ce) = check_poisoned(interp_run, ops, weights, act, torch.zeros(4), {}, d["B"])
    assert torch.equal(ga, ca) and torch.equal(gs, cs) and ge == {} and ce == {}
    assert ga.numel() == act.numel() and ga[d["out"]:].abs().max() > 0
    x = act[: d["a"]].view(-1, d["lda"])[:, : d["cin"]]
    want = x @ weights[: d["N"] * d["cin"]].view(d["N"], d["cin"]).T + weights[d["N"] * d["cin"]: d["N"] * d["cin"] + d["N"]]
    assert (ga[d["out"]: d["out"] + want.numel()].view_as(want) - want).abs().max() < 1e-5


@pytest.mark.parametrize("planted,message,caught_by", [
    (_shifted_read, "depends on memory no operand owns", (NAN, GARBAGE)),
    (_zero_times_garbage, "depends on memory no operand owns", (NAN,)),
    (_store_behind_output, "wrote memory no operand owns", (NAN, GARBAGE)),
    (_fmax_with_neighbour, "depends on memory no operand owns", (GARBAGE,)),
])
def test_planted_runners_are_rejected_under_poison_and_accepted_under_zeros(planted, message, caught_by):
    ops, weights, act, d = _gemm()
    args = (planted, ops, weights, act, torch.zeros(4), {}, d["B"])
    check_poisoned(*args, fills=(ZERO,))              # zeros in nobody's floats: invisible -- what the suite's inputs hold
    with pytest.raises(AssertionError, match=message):
        check_poisoned(*args)                         # the default: NAN, then GARBAGE
    for fill in (NAN, GARBAGE):
        if fill in caught_by:
            with pytest.raises(AssertionError, match=f"{message} under {fill}.*k_gemm"):
                check_poisoned(*args, fills=(fill,))
        else:
            check_poisoned(*args, fills=(fill,))      # ... and why one poison is not enough


def test_unrepeatable_runner_is_named_before_anything_else():
    ops, weights, act, d = _gemm()
    calls = {"n": 0}

    def drifting(ops_, weights_, act_, shr_, ext_, B, n_shr=0):
        interp_run(ops_, weights_, act_, shr_, ext_, B, n_shr)
        calls["n"] += 1
        act_[ops_[0].out.off * B] += calls["n"]
    with pytest.raises(AssertionError, match=r"not repeatable: act\[\d+\].*#0 k_gemm"):
        check_poisoned(drifting, ops, weights, act, torch.zeros(4), {}, d["B"])
    assert calls["n"] == 2


def test_ext_buffers_nobody_views_pass_through_with_guards_only():
    """Hand-off flags / data handed in by a test: the interpreter never views them, so their contents are the caller's in every
    run (the flags' zero-at-allocation contract) and only the guard bands are watched."""
    ops, weights, act, d = _gemm()
    seen = []

    def runner(ops_, weights_, act_, shr_, ext_, B, n_shr=0):
        seen.append(ext_[3].clone())
        interp_run(ops_, weights_, act_, shr_, ext_, B, n_shr)
    flags = torch.zeros(64)
    flags[5] = 2.0
    (_, _, ge), _ = check_poisoned(runner, ops, weights, act, torch.zeros(4), {3: flags}, d["B"])
    assert len(seen) == 4 and all(torch.equal(s, flags) for s in seen) and torch.equal(ge[3], flags)

    def scribble(ops_, weights_, act_, shr_, ext_, B, n_shr=0):
        interp_run(ops_, weights_, act_, shr_, ext_, B, n_shr)
        ext_[3].as_strided((1,), (1,), ext_[3].storage_offset() + 64).zero_()       # one float behind the flags
    with pytest.raises(AssertionError, match=r"wrote memory no operand owns under NAN: ext\[3\]\[64\] \(guard band\)"):
        check_poisoned(scribble, ops, weights, act, torch.zeros(4), {3: flags}, d["B"])


# ---------------------------------------------------------------------------------------- whole compiled programs under poison
SHARED_MODES = ["bf16x3", "bf16x3-wide", "f32", "f32-layers", "bf16"]
HAS_256 = ("cfg1", "sparse")          # the cases with a 256-channel transformer level (MDT_OP_TF256: narrow / wide forms)


@functools.lru_cache(maxsize=None)
def _model(case):
    m = make_synth_model(case)
    return m, {k: v.detach().float().cpu() for k, v in m.unet.state_dict().items()}


def _compile(case, mode, rows, monkeypatch):
    m, sd = _model(case)
    gemm, _, form = mode.partition("-")
    monkeypatch.setenv("MDT_F32_FUSED", "0" if form == "layers" else "1")
    return compile_unet(m.unet.config, m.max_length, m.unet.config.ctx_max_length, sd, max_time_rows=4, gemm_mode=gemm,
                        tf256=form == "wide", rows=rows)


def _evaluate(cu, g, B, fixed, fill):
    """One evaluation of the compiled programs through the interpreter as the engine runs them -- time mapping, context,
    evaluation -- on an activation arena (and a per-row FiLM table) that holds `fill` where reserve() leaves torch.empty."""
    x, t, emb = (torch.from_numpy(g[k])[:B] for k in ("x", "t", "emb"))
    _, C, L = x.shape
    act, shr = fill_floats(fill, cu.act_floats * B, seed=1), torch.zeros(cu.shr_floats)
    xin, out = torch.zeros(B, L, cu.in_pad), torch.zeros(B, L, cu.in_pad)
    xin[:, :, :C] = x.transpose(1, 2)
    ext = {EXT_XIN: xin.view(-1), EXT_CTX: emb.contiguous().view(-1), EXT_OUT: out.view(-1)}
    if cu.rows:
        ext[EXT_FILM] = fill_floats(fill, B * cu.ss_total, seed=2)
    bufs = Buffers(cu.weights, act, shr, ext)
    if cu.rows:
        off = cu.act_named["c_noise"] * B
        act[off: off + B] = t
        run_program(cu.programs["time_rows"], bufs, B, B)
    else:
        shr[cu.shr["c_noise"]] = t[0]
        run_program(cu.programs["time"], bufs, B, 1)
        shr[cu.shr["ss_cur"]: cu.shr["ss_cur"] + cu.ss_total] = shr[cu.shr["ss_all"]: cu.shr["ss_all"] + cu.ss_total].clone()
    run_program(cu.programs["ctx_fixed" if fixed else "ctx"], bufs, B)
    name = ("eval_rows" if cu.rows else "eval") + ("_fixed" if fixed else "")
    run_program(cu.programs[name], bufs, B)
    return out


def _programs_under_poison(cu, case):
    g = load_golden(f"{case}_unet.npz")
    for B in (1, 2):
        for fixed in (False, True):
            base = _evaluate(cu, g, B, fixed, ZERO)
            assert torch.isfinite(base).all() and base.abs().max() > 0
            for fill in (NAN, GARBAGE):
                got = _evaluate(cu, g, B, fixed, fill)
                assert not torch.isnan(got).any(), (case, B, fixed, fill)
                assert torch.equal(got.view(torch.int32), base.view(torch.int32)), (case, B, fixed, fill)


@pytest.mark.parametrize("case,mode", [(c, m) for c in ("tiny", "pd22", "cfg3", "cfg1", "sparse", "full") for m in SHARED_MODES
                                       if m != "bf16x3-wide" or c in HAS_256])
def test_shared_row_programs_do_not_depend_on_the_arena(case, mode, monkeypatch):
    """The lowering -- slot liveness in the compiler's arena, padded channel columns -- at the level of the op semantics: no op
    reads a slot before something wrote it."""
    _programs_under_poison(_compile(case, mode, False, monkeypatch), case)


@pytest.mark.parametrize("mode", ["bf16x3", "f32"])
@pytest.mark.parametrize("case", ["tiny", "pd22", "cfg3", "cfg1", "sparse", "full"])
def test_per_row_programs_do_not_depend_on_the_arena_or_the_film_table(case, mode, monkeypatch):
    cu = _compile(case, mode, True, monkeypatch)
    assert cu.rows and {"time_rows", "eval_rows", "eval_rows_fixed"} <= set(cu.programs)
    _programs_under_poison(cu, case)
