"""-m gpu: AEulerSampler / KarrasSampler on the fused path against golden vectors from the real reference
(tests/golden/make_golden_samplers.py), the four update kernels alone against the reference's arithmetic, and the
structure, sharding and per-step seams of the two loops.

Tolerance: the project's contract, <= 1e-4 max-abs deviation from the fp32 CPU reference on identical noise, on final
samples and intermediate sampler states, in all three product modes.  Every figure is printed before it is asserted
(`pytest -s` shows them; DESIGN.md section 5 carries the measured values).
"""
import os

import pytest
import torch

from conftest import load_golden
from elem_ref import dyn_scale_ref
from gpu_util import DEV, make_model, rnd
from helpers import noise_fns, to_t
from moleculediffusiontransformer_amd import ADPM2Sampler, AEulerSampler, KarrasSampler, KarrasSchedule, NoiseSource
from moleculediffusiontransformer_amd import runtime as rt

pytestmark = pytest.mark.gpu
TOL = 1e-4


@pytest.fixture(scope="module", params=["bf16x3", "f32", "f32-layers"])
def models(request):
    """The three product modes of test_gpu_parity.py's fixture of the same name: split-bf16 MFMA (default), exact fp32 MFMA on the
    same fused program, and the exact mode's layer-by-layer form (MDT_F32_FUSED=0)."""
    cache = {}
    mode, _, form = request.param.partition("-")
    old = os.environ.get("MDT_F32_FUSED")
    os.environ["MDT_F32_FUSED"] = "0" if form == "layers" else "1"      # read when an engine is compiled

    def get(case):
        if case not in cache:
            cache[case] = make_model(case)
            cache[case].gemm_mode = mode
        return cache[case]
    get.mode = request.param
    yield get
    if old is None:
        del os.environ["MDT_F32_FUSED"]
    else:
        os.environ["MDT_F32_FUSED"] = old


def sampler_of(g):
    name = str(g["sampler"])
    return AEulerSampler() if name == "aeuler" else KarrasSampler(*[float(v) for v in g["sampler_params"]])


def explicit(tag, shape):
    init, step = noise_fns(tag, shape)
    return init, NoiseSource(init=init, steps=lambda i: step(i, init))


PARITY = [
    ("tiny_b3_t8_aeuler", "tiny", (1, 7), 0.0),
    ("tiny_b3_t8_aeuler_cfg2", "tiny", (), 0.0),
    ("tiny_b3_t8_karras40_cfg2", "tiny", (1, 7), 0.0),
    ("tiny_b3_t8_karras0", "tiny", (), 0.0),
    ("pd22_b2_t6_aeuler", "pd22", (), 0.0),
    ("cfg3_b2_t10_aeuler", "cfg3", (), 0.0),
    ("cfg1_b2_t12_cfg7p5_aeuler", "cfg1", (), 0.0),
    ("cfg1_b2_t12_cfg7p5_karras4", "cfg1", (), 0.0),
    ("cfg1_b4_t32_aeuler", "cfg1", (1, 16, 31), 0.0),
    ("cfg1_b4_t32_karras4", "cfg1", (1, 16, 31), 0.0),
    ("tiny_dyn_t6_aeuler", "tiny", (), 0.9),          # KDiffusion_mod.dynamic_threshold = 0.9, as tests/golden/dynthr.npz
]


@pytest.mark.parametrize("name,case,want,dyn", PARITY)
def test_sample_matches_reference(models, name, case, want, dyn):
    """Measured on an MI355X (max-abs against the reference, final sample; bf16x3 / f32 / f32-layers): see DESIGN.md section 5."""
    g = load_golden(f"{name}_sample.npz")
    m = models(case)
    out_ref = to_t(g["out"])
    init, ns = explicit(name, tuple(out_ref.shape))
    trace = {"want": want}
    kd = m.diffusion.diffusion
    assert kd.dynamic_threshold == 0.0
    kd.dynamic_threshold = dyn
    try:
        out = m.sample(to_t(g["seq"]), DEV, cond_scale=float(g["cond_scale"]), timesteps=int(g["timesteps"]), clamp=False,
                       noise=ns, trace=trace, sampler=sampler_of(g))
    finally:
        kd.dynamic_threshold = 0.0
    assert out.shape == out_ref.shape and out.device.type == "cuda" and not out.requires_grad
    errs = {s: float((trace[s].cpu() - to_t(g[f"x_step{s}"])).abs().max()) for s in want}
    err = float((out.cpu() - out_ref).abs().max())
    print(f"\nPARITY {name} {models.mode} final {err:.3e} " + " ".join(f"step{s} {e:.3e}" for s, e in errs.items()))
    for s, e in errs.items():
        assert e < TOL, (name, s, e)
    assert err < TOL, (name, err)
    if name.endswith("karras0"):
        # KarrasSampler() as the reference writes it does not move without churn (diffusion.py:434): a known answer
        assert torch.equal(out.cpu(), float(KarrasSchedule(0.001, 9.0, 3.0)(int(g["timesteps"]))[0]) * init)
        assert torch.equal(out.cpu(), out_ref)
    assert m._engine.handoff_status() == 0


# ----------------------------------------------------------------------------------------------------------------------
# the kernels alone
# ----------------------------------------------------------------------------------------------------------------------
SHAPES = [(5, 22, 32, 32), (3, 1, 32, 16), (2, 16, 64, 16)]
DYN_TOL = 1e-6        # what test_gpu_seams.py::test_dynamic_thresholding_on_the_gpu_path asks of the dynamic clip


def _clip(raw, scale):
    """clip() of the denoised value: static clamp, or -- scale (B,) from mdt_dyn_scale -- clamp to [-s, s] and divide."""
    if scale is None:
        return raw.clamp(-1.0, 1.0)
    s = scale.view(-1, 1, 1)
    return torch.maximum(torch.minimum(raw, s), -s) / s


def _dyn(lib, gx, gp, c_skip, c_out, dims, st, on):
    if not on:
        return None
    B, C, L, Cp = dims
    ds = torch.empty(B, device=DEV)
    rt.check(lib.mdt_dyn_scale(rt.ptr(gx), rt.ptr(gp), rt.ptr(ds), c_skip, c_out, 0.9, B, C, L, Cp, st))
    # the expected scale is the bit-level host reference's (tests/elem_ref.py), which the kernel's has to equal
    want = dyn_scale_ref(gx.cpu(), gp.cpu(), c_skip, c_out, 0.9)
    assert torch.equal(ds.cpu(), want), (ds.cpu(), want)
    return want.to(DEV)


def _same(got, want, dyn):
    if dyn:
        return float((got - want).abs().max()) < DYN_TOL
    return torch.equal(got, want)


def _xin_ok(xin, want_cl, C):
    """xin (B, L, Cp) token-major: the first C channels equal want (B, C, L) transposed, the padding is zero."""
    return torch.equal(xin[:, :, :C], want_cl.transpose(1, 2)) and float(xin[:, :, C:].abs().sum()) == 0.0


@pytest.mark.parametrize("dyn", [False, True])
@pytest.mark.parametrize("dims", SHAPES)
def test_aeuler_kernel_matches_reference_arithmetic(dims, dyn):
    lib = rt.load_library()
    B, C, L, Cp = dims
    x, nz, pred = rnd(B, C, L, seed=1) * 3, rnd(B, C, L, seed=3), rnd(B, L, Cp, seed=4)
    c_skip, c_out, c_in, sigma, dt, up = 0.31, 0.095, 3.3, 0.29, -0.11, 0.17
    gx, gnz, gp = (t.to(DEV).contiguous() for t in (x, nz, pred))
    p = pred[:, :, :C].transpose(1, 2)
    with torch.cuda.device(DEV):
        st = rt.current_stream()
        ds = _dyn(lib, gx, gp, c_skip, c_out, dims, st, dyn)
        den = _clip(c_skip * x + c_out * p, None if ds is None else ds.cpu())
        want = x + ((x - den) / torch.tensor(sigma)) * torch.tensor(dt)
        want = want + nz * torch.tensor(up)
        # with xin_next
        x1, xin = gx.clone(), torch.full((B, L, Cp), 7.0, device=DEV)
        rt.check(lib.mdt_aeuler_next(rt.ptr(x1), rt.ptr(gp), rt.ptr(gnz), rt.ptr(xin), c_skip, c_out, sigma, dt, up, c_in, 0, 0, 0,
                                     B, C, L, Cp, 0, rt.ptr(ds), st))
        assert _same(x1.cpu(), want, dyn)
        assert _xin_ok(xin.cpu(), torch.tensor(c_in) * x1.cpu(), C)
        # last update of a call: no xin_next, the decode fused in
        x2, tok = gx.clone(), torch.full((B, L), -1, dtype=torch.int32, device=DEV)
        rt.check(lib.mdt_aeuler_next(rt.ptr(x2), rt.ptr(gp), rt.ptr(gnz), 0, c_skip, c_out, sigma, dt, up, 0.0, 0, 0, 0,
                                     B, C, L, Cp, rt.ptr(tok), rt.ptr(ds), st))
        assert torch.equal(x2, x1)
        assert torch.equal(tok.cpu().long(), x2.cpu().permute(0, 2, 1).argmax(dim=2))
        # the counter-based form equals the explicit form fed with mdt_init_noise's draws of the same (seed, draw index, sample0)
        seed, draw, s0 = 1234, 5, 7
        gz = torch.empty_like(gx)
        rt.check(lib.mdt_init_noise(rt.ptr(gz), 0, 1.0, seed, draw, s0, B, C, L, st))
        xa, xb = gx.clone(), gx.clone()
        rt.check(lib.mdt_aeuler_next(rt.ptr(xa), rt.ptr(gp), 0, 0, c_skip, c_out, sigma, dt, up, 0.0, seed, draw, s0,
                                     B, C, L, Cp, 0, rt.ptr(ds), st))
        rt.check(lib.mdt_aeuler_next(rt.ptr(xb), rt.ptr(gp), rt.ptr(gz), 0, c_skip, c_out, sigma, dt, up, 0.0, 0, 0, 0,
                                     B, C, L, Cp, 0, rt.ptr(ds), st))
        assert torch.equal(xa, xb) and not torch.equal(xa, x1)
        # the ABI refuses tokens together with xin_next, as mdt_adpm2_next does
        assert lib.mdt_aeuler_next(rt.ptr(x2), rt.ptr(gp), rt.ptr(gnz), rt.ptr(xin), c_skip, c_out, sigma, dt, up, c_in, 0, 0, 0,
                                   B, C, L, Cp, rt.ptr(tok), 0, st) != 0


@pytest.mark.parametrize("dyn", [False, True])
@pytest.mark.parametrize("dims", SHAPES)
def test_karras_kernels_match_reference_arithmetic(dims, dyn):
    lib = rt.load_library()
    B, C, L, Cp = dims
    x, nz = rnd(B, C, L, seed=1) * 3, rnd(B, C, L, seed=3)
    pred, pred2 = rnd(B, L, Cp, seed=4), rnd(B, L, Cp, seed=5)
    ns, s_noise, c_in = 0.37, 1.003, 3.3
    c_skip, c_out, sigma_hat, dt = 0.31, 0.095, 0.41, -0.12
    c_skip2, c_out2, sigma_next, half = 0.45, 0.08, 0.29, -0.06
    gx, gnz, gp, gp2 = (t.to(DEV).contiguous() for t in (x, nz, pred, pred2))
    p, p2 = pred[:, :, :C].transpose(1, 2), pred2[:, :, :C].transpose(1, 2)
    with torch.cuda.device(DEV):
        st = rt.current_stream()
        # churn: x_hat = x + ns * (s_noise * noise)
        x_hat = x + torch.tensor(ns) * (torch.tensor(s_noise) * nz)
        gh, xin = torch.empty_like(gx), torch.full((B, L, Cp), 7.0, device=DEV)
        rt.check(lib.mdt_karras_hat(rt.ptr(gx), rt.ptr(gnz), rt.ptr(gh), rt.ptr(xin), ns, s_noise, c_in, 0, 0, 0, B, C, L, Cp, st))
        assert torch.equal(gh.cpu(), x_hat)
        assert _xin_ok(xin.cpu(), torch.tensor(c_in) * x_hat, C)
        inplace = gx.clone()
        rt.check(lib.mdt_karras_hat(rt.ptr(inplace), rt.ptr(gnz), rt.ptr(inplace), rt.ptr(xin), ns, s_noise, c_in, 0, 0, 0,
                                    B, C, L, Cp, st))
        assert torch.equal(inplace, gh)
        seed, draw, s0 = 99, 3, 11
        gz, ha, hb = torch.empty_like(gx), torch.empty_like(gx), torch.empty_like(gx)
        rt.check(lib.mdt_init_noise(rt.ptr(gz), 0, 1.0, seed, draw, s0, B, C, L, st))
        rt.check(lib.mdt_karras_hat(rt.ptr(gx), 0, rt.ptr(ha), rt.ptr(xin), ns, s_noise, c_in, seed, draw, s0, B, C, L, Cp, st))
        rt.check(lib.mdt_karras_hat(rt.ptr(gx), rt.ptr(gz), rt.ptr(hb), rt.ptr(xin), ns, s_noise, c_in, 0, 0, 0, B, C, L, Cp, st))
        assert torch.equal(ha, hb) and not torch.equal(ha, gh)
        # without churn the stage is the identity on x (the draw is multiplied by 0)
        rt.check(lib.mdt_karras_hat(rt.ptr(gx), rt.ptr(gnz), rt.ptr(ha), rt.ptr(xin), 0.0, s_noise, c_in, 0, 0, 0, B, C, L, Cp, st))
        assert torch.equal(ha, gx)

        # Euler move from sigma_hat to sigma_next
        ds = _dyn(lib, gh, gp, c_skip, c_out, dims, st, dyn)
        den = _clip(c_skip * x_hat + c_out * p, None if ds is None else ds.cpu())
        d = (x_hat - den) / torch.tensor(sigma_hat)
        x_next = x_hat + torch.tensor(dt) * d
        gd, gn = torch.empty_like(gx), torch.empty_like(gx)
        xin.fill_(7.0)
        rt.check(lib.mdt_karras_mid(rt.ptr(gh), rt.ptr(gp), rt.ptr(gd), rt.ptr(gn), rt.ptr(xin), c_skip, c_out, sigma_hat, dt, c_in,
                                    B, C, L, Cp, 0, rt.ptr(ds), st))
        assert _same(gd.cpu(), d, dyn) and _same(gn.cpu(), x_next, dyn)
        assert _xin_ok(xin.cpu(), torch.tensor(c_in) * gn.cpu(), C)
        # sigma_next == 0: the move ends the step -- no xin_next, the decode fused in
        gd2, gn2, tok = torch.empty_like(gx), torch.empty_like(gx), torch.full((B, L), -1, dtype=torch.int32, device=DEV)
        rt.check(lib.mdt_karras_mid(rt.ptr(gh), rt.ptr(gp), rt.ptr(gd2), rt.ptr(gn2), 0, c_skip, c_out, sigma_hat, dt, 0.0,
                                    B, C, L, Cp, rt.ptr(tok), rt.ptr(ds), st))
        assert torch.equal(gd2, gd) and torch.equal(gn2, gn)
        assert torch.equal(tok.cpu().long(), gn2.cpu().permute(0, 2, 1).argmax(dim=2))

        # correction as the reference writes it: x = x_hat + half * (d + d')
        d_g, xn_g = gd.cpu(), gn.cpu()               # (from the kernel's own d and x_next, so that the stage is compared alone)
        ds2 = _dyn(lib, gn, gp2, c_skip2, c_out2, dims, st, dyn)
        den2 = _clip(c_skip2 * xn_g + c_out2 * p2, None if ds2 is None else ds2.cpu())
        d_prime = (xn_g - den2) / torch.tensor(sigma_next)
        want = x_hat + torch.tensor(half) * (d_g + d_prime)
        out, tok = torch.empty_like(gx), torch.full((B, L), -1, dtype=torch.int32, device=DEV)
        rt.check(lib.mdt_karras_next(rt.ptr(gh), rt.ptr(gn), rt.ptr(gd), rt.ptr(gp2), rt.ptr(out), c_skip2, c_out2, sigma_next, half,
                                     B, C, L, Cp, 0, rt.ptr(ds2), st))
        assert _same(out.cpu(), want, dyn)
        inplace = gh.clone()
        rt.check(lib.mdt_karras_next(rt.ptr(inplace), rt.ptr(gn), rt.ptr(gd), rt.ptr(gp2), rt.ptr(inplace), c_skip2, c_out2, sigma_next,
                                     half, B, C, L, Cp, rt.ptr(tok), rt.ptr(ds2), st))
        assert torch.equal(inplace, out)
        assert torch.equal(tok.cpu().long(), out.cpu().permute(0, 2, 1).argmax(dim=2))
        # half == 0 (no churn): the step returns x_hat
        rt.check(lib.mdt_karras_next(rt.ptr(gh), rt.ptr(gn), rt.ptr(gd), rt.ptr(gp2), rt.ptr(out), c_skip2, c_out2, sigma_next, 0.0,
                                     B, C, L, Cp, 0, rt.ptr(ds2), st))
        assert torch.equal(out, gh)
        # refused: a correction at sigma_next == 0, aliased buffers of the Euler move, tokens with xin_next
        assert lib.mdt_karras_next(rt.ptr(gh), rt.ptr(gn), rt.ptr(gd), rt.ptr(gp2), rt.ptr(out), c_skip2, c_out2, 0.0, half,
                                   B, C, L, Cp, 0, 0, st) != 0
        assert lib.mdt_karras_mid(rt.ptr(gh), rt.ptr(gp), rt.ptr(gd), rt.ptr(gh), rt.ptr(xin), c_skip, c_out, sigma_hat, dt, c_in,
                                  B, C, L, Cp, 0, 0, st) != 0
        assert lib.mdt_karras_mid(rt.ptr(gh), rt.ptr(gp), rt.ptr(gd), rt.ptr(gn), rt.ptr(xin), c_skip, c_out, sigma_hat, dt, c_in,
                                  B, C, L, Cp, rt.ptr(tok), 0, st) != 0


# ----------------------------------------------------------------------------------------------------------------------
# structure, sharding, seams
# ----------------------------------------------------------------------------------------------------------------------
class CountingTimer:
    def __init__(self):
        self.starts = self.stops = 0

    def start(self):
        self.starts += 1

    def stop(self):
        self.stops += 1


@pytest.mark.parametrize("scale", [1.0, 2.0])
def test_evaluations_per_call(scale):
    """AEuler: T - 1 evaluations; Karras and ADPM2: 2 (T - 1).  The timer brackets one guided evaluation, whether it runs as a
    doubled batch or as two passes."""
    m = make_model("tiny")
    g = load_golden("tiny_b3_t8_aeuler_sample.npz")
    seq, T = to_t(g["seq"]), 8
    for smp, n in ((AEulerSampler(), T - 1), (KarrasSampler(0.05, 5.0, 40.0, 1.003), 2 * (T - 1)), (KarrasSampler(), 2 * (T - 1)),
                   (ADPM2Sampler(rho=1), 2 * (T - 1))):
        t = CountingTimer()
        out = m.sample(seq, DEV, cond_scale=scale, timesteps=T, noise=NoiseSource(seed=3), timer=t, sampler=smp)
        assert (t.starts, t.stops) == (n, n), (type(smp).__name__, t.starts)
        assert out.shape == (3, 16, 32) and bool(torch.isfinite(out).all())
        # the timed route and the plain call (ONE custom op) are the same loop
        plain = m.sample(seq, DEV, cond_scale=scale, timesteps=T, noise=NoiseSource(seed=3), sampler=smp)
        assert torch.equal(plain, out)
        assert m._engine.handoff_status() == 0
    # num_steps == 1: no step at all, the scaled first draw (a one-entry KarrasSchedule is 0 / 0: a hand-made one); an empty batch
    def two(num_steps, device=None):
        return torch.tensor([2.0, 0.0])
    for smp in (AEulerSampler(), KarrasSampler(s_churn=4.0)):
        one = m.sample(seq, DEV, cond_scale=scale, timesteps=1, noise=NoiseSource(seed=3), sampler=smp, sigma_schedule=two)
        ref = m.sample(seq, DEV, cond_scale=scale, timesteps=1, noise=NoiseSource(seed=3), sigma_schedule=two)
        assert torch.equal(one, ref) and bool(torch.isfinite(one).all()) and float(one.abs().max()) > 1.0
        assert m.sample(seq[:0], DEV, cond_scale=scale, timesteps=4, sampler=smp).shape == (0, 16, 32)


@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("smp", [AEulerSampler(), KarrasSampler(0.05, 5.0, 40.0, 1.003)], ids=["aeuler", "karras40"])
def test_sample_tokens_decodes_the_returned_sample(smp, clamp):
    m = make_model("tiny")
    seq = to_t(load_golden("tiny_b3_t8_aeuler_sample.npz")["seq"])
    tok, x = m.sample_tokens(seq, DEV, cond_scale=1.0, timesteps=8, clamp=clamp, noise=NoiseSource(seed=11), return_sample=True,
                             sampler=smp)
    assert tok.dtype == torch.int64 and tok.shape == (3, 32) and tok.device.type == "cuda"
    assert torch.equal(tok, torch.argmax(torch.permute(x, (0, 2, 1)), dim=2))
    if clamp:
        assert float(x.abs().max()) <= 1.0
    again = m.sample(seq, DEV, cond_scale=1.0, timesteps=8, clamp=clamp, noise=NoiseSource(seed=11), sampler=smp)
    assert torch.equal(again, x)
    assert m._engine.handoff_status() == 0


@pytest.mark.parametrize("smp", [AEulerSampler(), KarrasSampler(0.05, 5.0, 40.0, 1.003)], ids=["aeuler", "karras40"])
def test_shards_equal_the_whole_batch_bit_for_bit(smp):
    from moleculediffusiontransformer_amd.synth import synth_normal
    m = make_model("tiny")
    m.kernel_choice = "narrow"
    seq = synth_normal("samplers/shard_seq", (6, 12))
    whole = m.sample(seq, DEV, cond_scale=1.0, timesteps=6, noise=NoiseSource(seed=77, sample0=0), sampler=smp)
    lo = m.sample(seq[:3], DEV, cond_scale=1.0, timesteps=6, noise=NoiseSource(seed=77, sample0=0), sampler=smp)
    hi = m.sample(seq[3:], DEV, cond_scale=1.0, timesteps=6, noise=NoiseSource(seed=77, sample0=3), sampler=smp)
    assert torch.equal(torch.cat([lo, hi]), whole)
    assert not torch.equal(lo, hi)
    assert m._engine.handoff_status() == 0


class StepEuler(AEulerSampler):
    """A subclass with its own step(): honoured, i.e. the per-step path (one fn call + one mdt_adpm2_euler launch per step)."""

    def __init__(self, draws):
        super().__init__()
        self.draws, self.calls = draws, 0

    def step(self, x, fn, sigma, sigma_next):
        self.calls += 1
        return super().step(x, fn, sigma, sigma_next, noise=self.draws(self.calls - 1, x))


class StepKarras(KarrasSampler):
    def __init__(self, draws, *params):
        super().__init__(*params)
        self.draws, self.calls = draws, 0

    def step(self, x, fn, sigma, sigma_next, gamma):
        self.calls += 1
        return super().step(x, fn, sigma, sigma_next, gamma, noise=self.draws(self.calls - 1, x))


@pytest.mark.parametrize("name", ["tiny_b3_t8_aeuler_cfg2", "tiny_b3_t8_karras40_cfg2"])
def test_per_step_path_of_a_subclass_matches_reference(name):
    g = load_golden(f"{name}_sample.npz")
    m = make_model("tiny")
    init, step = noise_fns(name, tuple(g["out"].shape))
    T = int(g["timesteps"])
    if str(g["sampler"]) == "aeuler":
        smp = StepEuler(step)
    else:
        smp = StepKarras(step, *[float(v) for v in g["sampler_params"]])
    out = m.sample(to_t(g["seq"]), DEV, cond_scale=float(g["cond_scale"]), timesteps=T, clamp=False, noise=init.to(DEV), sampler=smp)
    assert smp.calls == T - 1
    err = float((out.cpu() - to_t(g["out"])).abs().max())
    print(f"\nSEAM {name} per-step {err:.3e}")
    assert err < TOL
    # the final clamp is applied exactly once on either path
    smp.calls = 0
    clamped = m.sample(to_t(g["seq"]), DEV, cond_scale=float(g["cond_scale"]), timesteps=T, clamp=True, noise=init.to(DEV), sampler=smp)
    assert torch.equal(clamped, out.clamp(-1.0, 1.0))
    _, ns = explicit(name, tuple(g["out"].shape))
    fused = m.sample(to_t(g["seq"]), DEV, cond_scale=float(g["cond_scale"]), timesteps=T, clamp=True, noise=ns,
                     sampler=type(smp).__mro__[1](*[float(v) for v in g["sampler_params"]]))
    assert float(fused.abs().max()) <= 1.0 and float((fused.cpu() - to_t(g["out"]).clamp(-1.0, 1.0)).abs().max()) < TOL
    # a NoiseSource drives the fused loop only
    for plain in (AEulerSampler(), KarrasSampler()):
        with pytest.raises(TypeError, match="NoiseSource drives the fused path only"):
            plain(NoiseSource(seed=1), fn=lambda x, sigma: x, sigmas=torch.tensor([1.0, 0.5, 0.0]), num_steps=2)
    with pytest.raises(TypeError, match="NoiseSource drives the fused path only"):
        m.sample(to_t(g["seq"]), DEV, cond_scale=1.0, timesteps=T, noise=ns, sampler=smp)
    assert m._engine.handoff_status() == 0
