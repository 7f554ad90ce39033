"""CPU: AEulerSampler / KarrasSampler class surface, their host plans against scalars recorded from the real reference
(tests/golden/sampler_scalars.npz, bit for bit), the dispatch predicate of the fused loop and the new op's shape inference."""
import inspect
import math

import numpy as np
import pytest
import torch

from conftest import load_golden
import moleculediffusiontransformer_amd as M
from moleculediffusiontransformer_amd import (ADPM2Sampler, AEulerSampler, DiffusionSampler, KarrasSampler, KarrasSchedule,
                                              NoiseSource)
from moleculediffusiontransformer_amd import diffusion as D
from moleculediffusiontransformer_amd.diffusion import aeuler_plan, fused_sampler_kind, karras_plan, plan_time_rows

SCHEDULE = dict(sigma_min=0.001, sigma_max=9.0, rho=3.0)


def bits(values):
    return np.asarray(values, dtype=np.float32).view(np.uint32)


def is_f32(v):
    return float(np.float32(v)) == v or math.isinf(v)


@pytest.mark.parametrize("T", [8, 12, 64])
def test_aeuler_plan_equals_the_reference_scalars_bit_for_bit(T):
    g = load_golden("sampler_scalars.npz")
    smp = AEulerSampler()
    sigmas, steps = aeuler_plan(T, KarrasSchedule(**SCHEDULE), smp, 0.5)
    assert np.array_equal(bits(sigmas.numpy()), bits(g[f"sigmas_{T}"])) and len(steps) == T - 1
    ups, downs = zip(*(smp.get_sigmas(sigmas[i], sigmas[i + 1]) for i in range(T - 1)))
    assert np.array_equal(np.array(ups, dtype=np.float64), g[f"ae_up_{T}"])               # doubles, exactly
    assert np.array_equal(np.array(downs, dtype=np.float64), g[f"ae_down_{T}"])
    assert np.array_equal(bits([s.dt for s in steps]), bits(g[f"ae_dt_{T}"]))
    assert np.array_equal(bits([s.sigma_up for s in steps]), bits(g[f"ae_up_{T}"].astype(np.float32)))
    assert np.array_equal(bits([s.sigma for s in steps]), bits(g[f"sigmas_{T}"][:T - 1]))
    assert all(is_f32(v) for s in steps for v in (s.sigma, s.sigma_up, s.dt, s.w.c_skip, s.w.c_out, s.w.c_in, s.w.c_noise))
    for s in (steps[0], steps[-1]):
        assert s.w == D.scale_weights(torch.tensor(s.sigma), 0.5)
    assert len(plan_time_rows(steps)) == T - 1                                            # one evaluation per step
    assert aeuler_plan(T, KarrasSchedule(**SCHEDULE), AEulerSampler(), 0.5)[1] is steps   # cached like adpm2_plan


@pytest.mark.parametrize("key", ["k40", "k4"])
@pytest.mark.parametrize("T", [8, 12, 64])
def test_karras_plan_equals_the_reference_scalars_bit_for_bit(T, key):
    g = load_golden("sampler_scalars.npz")
    params = [float(v) for v in g[f"{key}_params"]]
    sigmas, steps = karras_plan(T, KarrasSchedule(**SCHEDULE), KarrasSampler(*params), 0.5)
    assert len(steps) == T - 1
    for name, field in (("gamma", "gamma"), ("sigma_hat", "sigma_hat"), ("dt", "dt"), ("half", "half")):
        assert np.array_equal(bits([getattr(s, field) for s in steps]), bits(g[f"{key}_{name}_{T}"])), name
    assert np.array_equal(bits([s.noise_scale for s in steps]), bits(g[f"{key}_noise_{T}"].astype(np.float32)))
    assert np.array_equal(bits([s.s_noise for s in steps]), bits([params[3]] * (T - 1)))
    churn = min(params[2] / T, math.sqrt(2) - 1)
    assert {float(np.float32(churn)), 0.0} == {s.gamma for s in steps}               # both values of torch.where occur
    assert (churn == params[2] / T) == (key == "k4" and T > 8)                        # ... and both arms of the min over the cases
    assert steps[0].gamma == 0.0 and steps[0].sigma_hat == 9.0                        # sigma 9.0 lies outside [s_tmin, s_tmax]
    # two evaluations per step, at sigma_hat and sigma_next alternately; sigma_next never reaches the schedule's padded 0
    assert not any(s.euler_only for s in steps) and steps[-1].sigma_next == float(g[f"sigmas_{T}"][T - 1]) > 0.0
    assert [(s.row_hat, s.row_next) for s in steps] == [(2 * i, 2 * i + 1) for i in range(T - 1)]
    rows = plan_time_rows(steps)
    assert len(rows) == 2 * (T - 1)
    want = [v for s in steps for v in (D.scale_weights(torch.tensor(s.sigma_hat), 0.5).c_noise,
                                       D.scale_weights(torch.tensor(s.sigma_next), 0.5).c_noise)]
    assert np.array_equal(bits(rows), bits(want))
    if key == "k40" and T == 8:          # the evaluated sigmas recorded from the reference's denoise_fn calls
        ev = [v for s in steps for v in (s.sigma_hat, s.sigma_next)]
        assert np.allclose(ev, [9.0, 5.80497, 5.80497, 3.47276, 4.91123, 1.86758, 2.64115, 0.85361, 1.20719, 0.29506, 0.41728,
                                0.05612, 0.07937, 0.001], rtol=0, atol=6e-6)


def test_karras_plan_without_churn_and_with_a_final_zero_sigma():
    sigmas, steps = karras_plan(8, KarrasSchedule(**SCHEDULE), KarrasSampler(), 0.5)
    assert all(s.gamma == 0.0 and s.sigma_hat == s.sigma and s.noise_scale == 0.0 and s.half == 0.0 for s in steps)
    # a hand-made evaluated schedule that ends in 0: the last step is the Euler move alone and has ONE time row (no log(0))
    hand = torch.tensor([4.0, 1.0, 0.25, 0.0, 0.0])
    _, steps = karras_plan(4, hand, KarrasSampler(0.0, 10.0, 1.0, 1.0), 0.5)
    assert [s.euler_only for s in steps] == [False, False, True]
    assert steps[-1].w_next is None and steps[-1].row_next == -1 and steps[-1].sigma_next == 0.0
    assert [(s.row_hat, s.row_next) for s in steps] == [(0, 1), (2, 3), (4, -1)]
    rows = plan_time_rows(steps)
    assert len(rows) == 5 and all(math.isfinite(v) for v in rows)
    assert steps[-1].dt == -steps[-1].sigma_hat
    _, ae = aeuler_plan(4, hand, AEulerSampler(), 0.5)                          # AEuler: sigma_up = sigma_down = 0 there
    assert ae[-1].sigma_up == 0.0 and ae[-1].dt == -0.25 and len(plan_time_rows(ae)) == 3
    # the ADPM2 plan's rows are what the ADPM2 loop uploads
    _, ad = D.adpm2_plan(6, KarrasSchedule(**SCHEDULE), ADPM2Sampler(rho=1), 0.5)
    assert plan_time_rows(ad) == [v for s in ad for v in (s.w.c_noise, s.w_mid.c_noise)]


def test_class_surface_matches_the_reference_signatures():
    for name in ("AEulerSampler", "KarrasSampler"):
        assert getattr(M, name) is getattr(D, name)
    k = KarrasSampler()
    assert (k.s_tmin, k.s_tmax, k.s_churn, k.s_noise) == (0, float("inf"), 0.0, 1.0)
    k = KarrasSampler(0.05, 5.0, 40.0, 1.003)
    assert (k.s_tmin, k.s_tmax, k.s_churn, k.s_noise) == (0.05, 5.0, 40.0, 1.003)
    assert list(inspect.signature(KarrasSampler.__init__).parameters) == ["self", "s_tmin", "s_tmax", "s_churn", "s_noise"]
    assert list(inspect.signature(KarrasSampler.step).parameters)[:6] == ["self", "x", "fn", "sigma", "sigma_next", "gamma"]
    assert list(inspect.signature(AEulerSampler.step).parameters)[:5] == ["self", "x", "fn", "sigma", "sigma_next"]
    for cls in (AEulerSampler, KarrasSampler):
        assert list(inspect.signature(cls.forward).parameters) == ["self", "noise", "fn", "sigmas", "num_steps"]
        assert [t.alias for t in cls.diffusion_types] == ["k", "vk"] and issubclass(cls, M.Sampler)
        with pytest.raises(NotImplementedError, match="Inpainting not available with current sampler"):
            cls().inpaint(None, None, None, None, 2, 1)
    up, down = AEulerSampler().get_sigmas(torch.tensor(2.0), torch.tensor(1.0))
    assert isinstance(up, float) and up == math.sqrt(0.75) and down == 0.5      # (fp32 tensor arithmetic under math.sqrt)
    m = M.QMDiffusion(max_length=32, pred_dim=16, channels=16, context_embedding_max_length=12, text_embed_dim=64,
                      embed_dim_position=64)
    for smp in (AEulerSampler(), KarrasSampler(s_churn=4.0)):
        ds = DiffusionSampler(m.diffusion.diffusion, sampler=smp, sigma_schedule=KarrasSchedule(**SCHEDULE), num_steps=4)
        assert ds.sampler is smp
    # the per-step path has no CPU implementation, as for ADPM2Sampler
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        AEulerSampler().step(torch.zeros(1, 16, 32), lambda x, sigma: x, 1.0, 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KarrasSampler().step(torch.zeros(1, 16, 32), lambda x, sigma: x, 1.0, 0.5, 0.0)
    with pytest.raises(TypeError, match="NoiseSource drives the fused path only"):
        AEulerSampler()(NoiseSource(seed=1), fn=lambda x, sigma: x, sigmas=torch.tensor([1.0, 0.5, 0.0]), num_steps=2)
    with pytest.raises(TypeError, match="NoiseSource drives the fused path only"):
        KarrasSampler()(NoiseSource(seed=1), fn=lambda x, sigma: x, sigmas=torch.tensor([1.0, 0.5, 0.0]), num_steps=2)


def test_dispatch_predicate_honours_a_subclass_that_overrides_step():
    class MyEuler(AEulerSampler):
        def step(self, x, fn, sigma, sigma_next, **kw):
            return super().step(x, fn, sigma, sigma_next, **kw)

    class MyKarras(KarrasSampler):
        def step(self, x, fn, sigma, sigma_next, gamma, **kw):
            return super().step(x, fn, sigma, sigma_next, gamma, **kw)

    class Renamed(AEulerSampler):
        pass

    class Mine(M.Sampler):
        pass

    assert fused_sampler_kind(ADPM2Sampler()) == "adpm2" and fused_sampler_kind(AEulerSampler()) == "aeuler"
    assert fused_sampler_kind(KarrasSampler()) == "karras" and fused_sampler_kind(Renamed()) == "aeuler"
    assert fused_sampler_kind(MyEuler()) is None and fused_sampler_kind(MyKarras()) is None and fused_sampler_kind(Mine()) is None
    # ... and forward() then never asks the denoiser for its fused loop
    class Fn:
        @property
        def fused(self):
            raise AssertionError("a subclass with its own step() must take the per-step path")

        def __call__(self, x, sigma):
            return x
    with pytest.raises(RuntimeError, match="no CPU fallback"):         # i.e. it reached step()
        MyEuler()(torch.zeros(1, 16, 32), fn=Fn(), sigmas=torch.tensor([1.0, 0.5, 0.0]), num_steps=2)
    from moleculediffusiontransformer_amd import ops
    assert ops.sampler_spec(AEulerSampler()) == (1, [])
    assert ops.sampler_spec(KarrasSampler(0.05, 5.0, 4.0, 1.003)) == (2, [0.05, 5.0, 4.0, 1.003])
    assert ops.sampler_spec(ADPM2Sampler(rho=1)) == (0, [1.0])
    with pytest.raises(TypeError, match="no fused loop"):
        ops.sampler_spec(MyEuler())


def test_every_fused_kind_round_trips_through_the_sample_with_arguments():
    """D.FUSED_SAMPLERS is the one table of kind -> class, parameters, plan, loop: what sampler_spec() says of a sampler of
    every kind, _make_sampler() turns back into that sampler."""
    from moleculediffusiontransformer_amd import ops
    samplers = (ADPM2Sampler(rho=3.0), AEulerSampler(), KarrasSampler(0.05, 5.0, 4.0, 1.003))
    assert [type(s) for s in samplers] == [k.cls for k in D.FUSED_SAMPLERS.values()]            # one of every kind
    for i, (s, (name, k)) in enumerate(zip(samplers, D.FUSED_SAMPLERS.items())):
        kind, params = ops.sampler_spec(s)
        assert kind == i == ops.SAMPLER_KINDS[name] and fused_sampler_kind(s) == name
        assert [getattr(k.cls(*params), n) for n in k.params] == params          # ... in the constructor's own order
        back = ops._make_sampler(kind, params)
        assert type(back) is type(s) and ops.sampler_spec(back) == (kind, params)
        assert [getattr(back, n) for n in k.params] == [getattr(s, n) for n in k.params]
        with pytest.raises(RuntimeError, match=f"sampler_kind {kind} with {len(params) + 1} parameters"):
            ops._make_sampler(kind, params + [1.0])
    with pytest.raises(RuntimeError) as e:
        ops._make_sampler(3, [])
    assert str(e.value) == ("mdt::sample_with: sampler_kind 3 with 0 parameters (0 = ADPM2 [rho], 1 = AEuler [], "
                            "2 = Karras [s_tmin, s_tmax, s_churn, s_noise])")
    with pytest.raises(RuntimeError, match="sampler_kind -1 with 1 parameters"):
        ops._make_sampler(-1, [1.0])


def test_sample_with_shape_inference_and_the_default_route(monkeypatch):
    from torch._subclasses.fake_tensor import FakeTensorMode
    from moleculediffusiontransformer_amd import ops

    class Eng:
        class c:
            length = 32
    eng = Eng()
    h = ops.register_engine(eng)
    with FakeTensorMode():
        emb = torch.empty(5, 12, 128)
        sig = torch.empty(9)
        for kind, params in ((1, []), (2, [0.05, 5.0, 4.0, 1.003])):
            x, tok = torch.ops.mdt.sample_with(emb, None, None, sig, h, 16, kind, params, 0.5, 2.0, False, 7, 0, True, 0.0)
            assert x.shape == (5, 16, 32) and x.dtype == torch.float32
            assert tok.shape == (5, 32) and tok.dtype == torch.int32
            x, tok = torch.ops.mdt.sample_with(emb, None, None, sig, h, 16, kind, params, 0.5, 1.0, True, 7, 0, False)
            assert x.shape == (5, 16, 32) and tok.shape == (0,) and tok.dtype == torch.int32
        pred, xh = torch.empty(5, 32, 16), torch.empty(5, 16, 32)
        a, b = torch.ops.mdt.aeuler_next(xh, pred, None, 0.1, 0.2, 1.0, -0.5, 0.3, 2.0, 1, 1, 0)
        assert a.shape == xh.shape and b.shape == pred.shape
        a, b = torch.ops.mdt.karras_hat(xh, None, 0.3, 1.0, 2.0, 16, 1, 1, 0)
        assert a.shape == xh.shape and b.shape == pred.shape
        assert [t.shape for t in torch.ops.mdt.karras_mid(xh, pred, 0.1, 0.2, 1.0, -0.5, 2.0)] == [xh.shape, xh.shape, pred.shape]
        assert torch.ops.mdt.karras_next(xh, xh, xh, pred, 0.1, 0.2, 0.5, -0.1).shape == xh.shape
    # sample(..., sampler=None, sigma_schedule=None) is today's call: ADPM2Sampler(rho=1) over KarrasSchedule(0.001, 9.0, 3.0)
    m = M.QMDiffusion(max_length=32, pred_dim=16, channels=16, context_embedding_max_length=12, text_embed_dim=64,
                      embed_dim_position=64)
    seen = {}

    def fake_sample(**kw):
        seen.update(kw)
        return "x"
    monkeypatch.setattr(m, "_embed", lambda seq, dev: torch.zeros(seq.shape[0], 12, 128))
    monkeypatch.setattr(m.diffusion, "sample", fake_sample)
    assert m.sample(torch.zeros(2, 12), "cpu", timesteps=5) == "x"
    s, k = seen["sampler"], seen["sigma_schedule"]
    assert type(s) is ADPM2Sampler and s.rho == 1 and fused_sampler_kind(s) == "adpm2"
    assert type(k) is KarrasSchedule and (k.sigma_min, k.sigma_max, k.rho) == (0.001, 9.0, 3.0) and seen["num_steps"] == 5
    mine, sched = AEulerSampler(), KarrasSchedule(0.01, 5.0, 7.0)
    m.sample(torch.zeros(2, 12), "cpu", timesteps=5, sampler=mine, sigma_schedule=sched)
    assert seen["sampler"] is mine and seen["sigma_schedule"] is sched
    m.sample_tokens(torch.zeros(2, 12), "cpu", timesteps=5, sampler=mine)
    assert seen["sampler"] is mine and type(seen["sigma_schedule"]) is KarrasSchedule and seen["tokens"] is not None
    for fn in (M.QMDiffusion.sample, M.QMDiffusionForward.sample, M.QMDiffusion.sample_tokens, M.AnalogDiffusionFull.sample,
               M.predict_properties_from_tokens, M.generate_and_validate):
        p = inspect.signature(fn).parameters
        assert all(p[n].kind is inspect.Parameter.KEYWORD_ONLY and p[n].default is None for n in ("sampler", "sigma_schedule")), fn
    # the ADPM2 route of the fused loop is still mdt::sample (exact type), the other two go through mdt::sample_with
    src = inspect.getsource(M.generative._FusedLoop.sample)
    assert "torch.ops.mdt.sample(" in src and "torch.ops.mdt.sample_with(" in src
