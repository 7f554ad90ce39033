"""-m gpu: a guidance scale per sample -- mdt_cfg_mix_rows bit for bit against the reference's expression, the fused loops against
fixtures recorded from the real reference (one run per distinct scale, rows stitched), and the per-sample call against the scalar
calls it replaces, bit for bit under a pinned kernel_choice.

Tolerance: 1e-4 max-abs on the sample against the reference, as every parity test; everything else is bitwise.
"""
import os

import pytest
import torch

from conftest import load_golden
from gpu_util import DEV, make_model, rnd
from helpers import noise_fns, to_t
from test_gpu_elem import FLAT, TRIP
import moleculediffusiontransformer_amd as M
from moleculediffusiontransformer_amd import ADPM2Sampler, AEulerSampler, KarrasSampler, NoiseSource, guidance_sweep, runtime as rt
from moleculediffusiontransformer_amd.synth import synth_normal

pytestmark = pytest.mark.gpu
TOL = 1e-4
SAMPLERS = {"adpm2": lambda: ADPM2Sampler(rho=1), "aeuler": AEulerSampler, "karras": lambda: KarrasSampler(0.05, 5.0, 40.0, 1.003)}


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same(a, b):
    """fp32 tensors of one shape, equal bit for bit."""
    return a.dtype == b.dtype == torch.float32 and a.shape == b.shape and torch.equal(bits(a), bits(b))


# ----------------------------------------------------------------------------------------------------------------------
# 1. the kernel, bit for bit
# ----------------------------------------------------------------------------------------------------------------------
KERNEL_SHAPES = {
    "flat_past_the_grid_cap": (FLAT[0], FLAT[1] * FLAT[2], False),       # 130 rows of 4096 float4s: 2,080 segments of 256 lanes
    "more_rows_than_65535": (65537, 64, False),                          # 16-lane segments, 16 per workgroup: 4,097 workgroups' worth
    "three_short_rows_in_place": (3, 64, True),
}


@pytest.mark.parametrize("shape", list(KERNEL_SHAPES))
def test_cfg_mix_rows_is_the_reference_expression_bit_for_bit(shape):
    """out[b] = scale[b] == 1 ? cond[b] : um[b] + (cond[b] - um[b]) * scale[b] in fp32 without contraction.  Rows at scale 1 carry
    NaN in uncond and return cond untouched (the reference skips guidance there, and u + (c - u) is not c in fp32)."""
    lib = rt.load_library()
    B, row, in_place = KERNEL_SHAPES[shape]
    if shape == "flat_past_the_grid_cap":
        assert B * row // 4 > TRIP and B * (row // 4 // 256) > 2048       # elements and segments both take a second trip
    cond, um = rnd(B, row, seed=5), rnd(B, row, seed=6)
    s = torch.tensor([1.0, 2.0, 7.5, 0.0, 0.5, 1.0, -1.5, 3.0]).repeat((B + 7) // 8)[:B].clone()
    s[-1] = 1.0 if B > 3 else 7.5                                        # the last row of the long shapes is a scale-1 row
    ones = s == 1
    assert bool(ones.any()) and not bool(ones.all())
    assert not torch.equal((um + (cond - um))[ones], cond[ones])         # what a kernel without the == 1 branch would return
    um[ones] = float("nan")
    want = torch.where(ones.view(-1, 1), cond, um + (cond - um) * s.view(-1, 1))
    assert not bool(torch.isnan(want).any())
    gc, gu, gs = cond.to(DEV), um.to(DEV), s.to(DEV)
    with torch.cuda.device(DEV):
        st = rt.current_stream()
        out = gc if in_place else torch.full((B, row), 7.0, device=DEV)
        rt.check(lib.mdt_cfg_mix_rows(rt.ptr(gc), rt.ptr(gu), rt.ptr(out), rt.ptr(gs), B, row, st))
        torch.cuda.synchronize()
    got = out.cpu()
    assert torch.equal(bits(got[-1]), bits(want[-1])), "the last row"
    assert torch.equal(bits(got), bits(want))
    assert torch.equal(bits(got[ones]), bits(cond[ones]))
    if not in_place:
        assert torch.equal(gc.cpu(), cond)
        # the op over the same entry point, any trailing shape
        shaped = torch.ops.mdt.cfg_mix_rows(gc.view(B, -1, 16), gu.view(B, -1, 16), gs)
        assert shaped.shape == (B, row // 16, 16) and torch.equal(bits(shaped.view(B, row)), bits(want))
    with pytest.raises(RuntimeError, match="scale holds"):
        torch.ops.mdt.cfg_mix_rows(gc, gu, gs[:-1])
    with pytest.raises(RuntimeError, match="shape mismatch"):
        torch.ops.mdt.cfg_mix_rows(gc, gu[:, :32], gs)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        torch.ops.mdt.cfg_mix_rows(gc, gu, s)


def test_cfg_mix_rows_equals_cfg_mix_row_by_row():
    """The arithmetic form and evaluation order are k_cfg_mix's: every row at a scale != 1 is mdt_cfg_mix's at that scale."""
    lib = rt.load_library()
    B, row = 6, 16 * 36                                                  # 144 float4s: a 256-lane segment with idle lanes
    cond, um = rnd(B, row, seed=7).to(DEV), rnd(B, row, seed=8).to(DEV)
    s = torch.tensor([2.0, 7.5, 0.0, 0.1, -3.0, 1.0000001])
    with torch.cuda.device(DEV):
        st = rt.current_stream()
        out = torch.empty_like(cond)
        rt.check(lib.mdt_cfg_mix_rows(rt.ptr(cond), rt.ptr(um), rt.ptr(out), rt.ptr(s.to(DEV)), B, row, st))
        for b in range(B):
            one = torch.empty(row, device=DEV)
            rt.check(lib.mdt_cfg_mix(rt.ptr(cond[b]), rt.ptr(um[b]), rt.ptr(one), float(s[b]), row, st))
            assert torch.equal(bits(one), bits(out[b])), b
        torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------------------
# 2. parity with the reference
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["bf16x3", "f32", "f32-layers"])
def models(request):
    """The three product-mode forms of test_gpu_parity.py: split-bf16 MFMA, exact fp32 MFMA on the fused program, and the exact
    mode's layer-by-layer form."""
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


def fixture_cases():
    g = load_golden("guidance_rows.npz")
    return [(str(n), str(m), str(s), str(t)) for n, m, s, t in zip(g["cases"], g["models"], g["samplers"], g["tags"])]


@pytest.mark.parametrize("name,model,sampler,tag", fixture_cases())
def test_fixture_parity(models, name, model, sampler, tag):
    """Row b of ONE per-sample call against row b of the reference's run at scales[b]."""
    g = {k[len(name) + 1:]: v for k, v in load_golden("guidance_rows.npz").items() if k.startswith(f"{name}_")}
    m = models(model)
    out_ref, scales, T = to_t(g["out"]), to_t(g["scales"]), int(g["timesteps"])
    B = out_ref.shape[0]
    init, step = noise_fns(tag, tuple(out_ref.shape))
    out = m.sample(to_t(g["seq"]), DEV, cond_scale=scales, timesteps=T, noise=NoiseSource(init=init, steps=lambda i: step(i, init)),
                   sampler=SAMPLERS[sampler]())
    assert out.dtype == torch.float32 and out.shape == out_ref.shape
    err = (out.cpu() - out_ref).abs().flatten(1).max(dim=1).values
    print(f"\nguidance_rows {name} [{models.mode}]: max|hip - reference| per row = {[f'{float(e):.2e}' for e in err]}")
    assert float(err.max()) < TOL
    eng = m._engine
    dual = eng.has_dual and B % eng.c.dual_multiple == 0
    print(f"guidance_rows {name} [{models.mode}]: doubled batch {dual} (engine has one: {eng.has_dual}, multiple {eng.c.dual_multiple})")
    assert eng.B == (2 * B if dual else B)
    if model == "cfg1":                              # B = 8: the doubled batch [samples | samples] where the engine has one
        assert dual == eng.has_dual
    else:                                            # B = 5: two passes over the batch
        assert not dual
    assert eng.handoff_status() == 0


# ----------------------------------------------------------------------------------------------------------------------
# 3. - 6. against the scalar calls, bit for bit
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cfg1():
    m = make_model("cfg1")
    m.kernel_choice = "narrow"
    return m


def row_scales(B):
    """B scales from {1, 2, 7.5}, each present, in no order that follows the rows."""
    s = torch.tensor([7.5, 1.0, 2.0, 2.0, 1.0, 7.5, 1.0, 2.0, 7.5, 7.5, 2.0, 1.0, 2.0, 7.5, 1.0, 1.0])[:B]
    assert set(s.tolist()) == {1.0, 2.0, 7.5}
    return s


def stitched(call, scales, order=(2.0, 7.5, 1.0)):
    """(the per-sample call, row b of the scalar call at scales[b] for every b): tensors, or tuples of tensors.  The guided scalar
    calls come first: they share the per-sample call's engine batch, so its captured graphs are replayed."""
    rows = call(scales)
    runs = {s: call(s) for s in order}
    pick = lambda k: torch.stack([(runs[float(s)][k] if k is not None else runs[float(s)])[b] for b, s in enumerate(scales)])   # noqa: E731
    if isinstance(rows, tuple):
        return rows, tuple(pick(k) for k in range(len(rows)))
    return rows, pick(None)


@pytest.mark.parametrize("B", [16, 12], ids=["B16_doubled_batch", "B12_two_passes"])
def test_rows_equal_the_scalar_calls_for_every_sampler(cfg1, B):
    m = cfg1
    seq, scales = synth_normal("gr_eq/seq", (16, 12))[:B], row_scales(B)
    for kind, make in SAMPLERS.items():
        rows, want = stitched(lambda cs: m.sample(seq, DEV, cond_scale=cs, timesteps=4, noise=NoiseSource(seed=31, sample0=5),
                                                  sampler=make()), scales)
        assert bool(torch.isfinite(rows).all()) and same(rows, want), kind
        assert not torch.equal(rows[0], m.sample(seq, DEV, cond_scale=1.0, timesteps=4, noise=NoiseSource(seed=31, sample0=5),
                                                 sampler=make())[0]), kind            # row 0 (scale 7.5) is guided
    eng = m._engine
    assert eng.handoff_status() == 0
    # the form of the per-sample call: the doubled batch at B = 16 where the engine has one, two passes at B = 12
    m.sample(seq, DEV, cond_scale=scales, timesteps=2, noise=NoiseSource(seed=31))
    assert m._engine is eng and eng.B == (2 * B if eng.has_dual and B == 16 else B)
    assert not eng.has_dual or (B % eng.c.dual_multiple == 0) == (B == 16)


@pytest.mark.parametrize("B", [16, 12], ids=["B16_doubled_batch", "B12_two_passes"])
def test_rows_equal_the_scalar_calls_for_tokens_inpainting_and_dynamic_threshold(cfg1, B):
    m = cfg1
    C, L = m.pred_dim, m.max_length
    seq, scales = synth_normal("gr_eq/seq", (16, 12))[:B], row_scales(B)
    # sample_tokens: the ids are the argmax of the returned sample
    (tok, x), (tok_w, x_w) = stitched(lambda cs: m.sample_tokens(seq, DEV, cond_scale=cs, timesteps=4, noise=NoiseSource(seed=32),
                                                                 return_sample=True), scales)
    assert same(x, x_w) and torch.equal(tok, tok_w) and tok.dtype == torch.int64
    assert torch.equal(tok, torch.argmax(torch.permute(x, (0, 2, 1)), dim=2))
    assert torch.equal(m.sample_tokens(seq, DEV, cond_scale=scales.tolist(), timesteps=4, noise=NoiseSource(seed=32)), tok)
    # inpaint_tokens and the dense inpaint()
    draft = torch.randint(0, C, (B, L), generator=torch.Generator().manual_seed(61))
    keep = torch.rand(B, L, generator=torch.Generator().manual_seed(62)) < 0.4
    (tok, x), (tok_w, x_w) = stitched(lambda cs: m.inpaint_tokens(seq, DEV, draft, keep, cond_scale=cs, timesteps=4, num_resamples=2,
                                                                  seed=33, sample0=2, return_sample=True), scales)
    assert same(x, x_w) and torch.equal(tok, tok_w) and torch.equal(tok.cpu()[keep], draft[keep])
    src, mask = M.one_hot_draft(draft, C).to(DEV), keep.unsqueeze(1).expand(-1, C, -1).contiguous().to(DEV)
    dense = m.inpaint(seq, DEV, cond_scale=scales, timesteps=4, num_resamples=2, inpaint=src, in_paint_mask=mask, seed=33, sample0=2)
    assert same(dense, x)
    # a model with dynamic thresholding.  clip() divides by max(quantile, 1), so the threshold differs from the static clamp only
    # where the 0.9 quantile of |denoised| passes 1.  At sigma_data 0.1 the synthetic model's denoised values stay below 0.5 at
    # every scale here (oracle, CPU: max 0.47) and the two calls would be one and the same; at sigma_data 1 (c_out ~ 1: the
    # network's own output range) the quantile is 1.2 ... 2.2 at each of the three scales from the second step on at the latest.
    kd = m.diffusion.diffusion
    sigma_data = kd.sigma_data
    kd.sigma_data, kd.dynamic_threshold = 1.0, 0.9
    try:
        rows, want = stitched(lambda cs: m.sample(seq, DEV, cond_scale=cs, timesteps=4, noise=NoiseSource(seed=34)), scales)
        assert bool(torch.isfinite(rows).all()) and same(rows, want)
        kd.dynamic_threshold = 0.0
        plain = m.sample(seq, DEV, cond_scale=scales, timesteps=4, noise=NoiseSource(seed=34))
    finally:
        kd.sigma_data, kd.dynamic_threshold = sigma_data, 0.0
    unchanged = [b for b in range(B) if torch.equal(plain[b], rows[b])]
    assert not unchanged, unchanged                                      # (the threshold was in force, in every row)
    assert m._engine.handoff_status() == 0


class CountingTimer:
    def __init__(self):
        self.starts = self.stops = 0

    def start(self):
        self.starts += 1

    def stop(self):
        self.stops += 1


def test_uniform_scales_are_the_float_call(cfg1):
    m = cfg1
    B, T = 16, 4
    seq = synth_normal("gr_eq/seq", (B, 12))
    ns = lambda: NoiseSource(seed=35, sample0=1)                          # noqa: E731
    for v in (2.0, 0.0, 1.0):
        want = m.sample(seq, DEV, cond_scale=v, timesteps=T, noise=ns())
        for form in (torch.full((B,), v), [v] * B, torch.full((B,), v, dtype=torch.float64).numpy()):
            assert same(m.sample(seq, DEV, cond_scale=form, timesteps=T, noise=ns()), want), v
    # all ones: not guided -- one evaluation of B rows per timer interval, 2 (T - 1) intervals for ADPM2, no doubled batch
    t = CountingTimer()
    out = m.sample(seq, DEV, cond_scale=torch.ones(B), timesteps=T, noise=ns(), timer=t)
    assert (t.starts, t.stops) == (2 * (T - 1), 2 * (T - 1)) and m._engine.B == B
    assert same(out, m.sample(seq, DEV, cond_scale=1.0, timesteps=T, noise=ns()))
    unguided_ms = m._engine                       # the same engine object serves both batches under the pinned choice
    t = CountingTimer()
    m.sample(seq, DEV, cond_scale=row_scales(B), timesteps=T, noise=ns(), timer=t)
    assert (t.starts, t.stops) == (2 * (T - 1), 2 * (T - 1)) and m._engine is unguided_ms
    assert m._engine.B == (2 * B if m._engine.has_dual else B)
    # the timed route of a per-sample call is the plain one
    assert same(m.sample(seq, DEV, cond_scale=row_scales(B), timesteps=T, noise=ns(), timer=CountingTimer()),
                m.sample(seq, DEV, cond_scale=row_scales(B), timesteps=T, noise=ns()))


def test_guidance_sweep_equals_the_scalar_calls(cfg1):
    m = cfg1
    B, scales = 4, [7.5, 1.0, 2.0, 7.5]
    seq = synth_normal("gr_sweep/seq", (B, 12))
    out = guidance_sweep(m, seq, scales, DEV, timesteps=4, noise=NoiseSource(seed=36, sample0=0))
    assert out.shape == (4, B, m.pred_dim, m.max_length)
    tok, x = guidance_sweep(m, seq, scales, DEV, tokens=True, timesteps=4, noise=NoiseSource(seed=36, sample0=0), return_sample=True)
    assert same(x, out) and tok.shape == (4, B, m.max_length) and torch.equal(tok, out.argmax(dim=2))
    for s, scale in enumerate(scales):
        want = m.sample(seq, DEV, cond_scale=scale, timesteps=4, noise=NoiseSource(seed=36, sample0=s * B))
        assert same(out[s], want), s
    assert not torch.equal(out[0], out[3])                                # the same scale, other samples of the stream
    shifted = guidance_sweep(m, seq, scales, DEV, timesteps=4, noise=NoiseSource(seed=36, sample0=7))
    assert same(shifted[2], m.sample(seq, DEV, cond_scale=2.0, timesteps=4, noise=NoiseSource(seed=36, sample0=7 + 2 * B)))
    assert guidance_sweep(m, seq, [], DEV, timesteps=4).shape == (0, B, m.pred_dim, m.max_length)


def test_edge_cases(cfg1):
    m = cfg1
    C, L = m.pred_dim, m.max_length
    seq = synth_normal("gr_eq/seq", (3, 12))
    draft, keep = torch.zeros(3, L, dtype=torch.long), torch.zeros(3, L, dtype=torch.bool)
    # an empty batch returns empty results
    assert m.sample(seq[:0], DEV, cond_scale=[], timesteps=4).shape == (0, C, L)
    assert m.sample(seq[:0], DEV, cond_scale=torch.empty(0), timesteps=4, sampler=AEulerSampler()).shape == (0, C, L)
    tok, x = m.sample_tokens(seq[:0], DEV, cond_scale=[], timesteps=4, return_sample=True)
    assert tok.shape == (0, L) and tok.dtype == torch.int64 and x.shape == (0, C, L)
    tok, x = m.inpaint_tokens(seq[:0], DEV, draft[:0], keep[:0], cond_scale=[], seed=1, return_sample=True)
    assert tok.shape == (0, L) and x.shape == (0, C, L) and tok.device.type == "cuda"
    # a wrong length, a second dimension, a NaN: ValueError, nothing evaluated (the engine's batch is as it was)
    m.sample(seq, DEV, cond_scale=1.0, timesteps=2, noise=NoiseSource(seed=1))
    eng, before = m._engine, m._engine.B
    for bad in ([1.0, 2.0], [1.0, 2.0, 3.0, 4.0], [[1.0, 2.0, 3.0]], [1.0, float("nan"), 2.0]):
        with pytest.raises(ValueError, match="cond_scale must"):
            m.sample(seq, DEV, cond_scale=bad, timesteps=4)
        with pytest.raises(ValueError, match="cond_scale must"):
            m.inpaint_tokens(seq, DEV, draft, keep, cond_scale=bad, timesteps=4, seed=1)
    assert m._engine is eng and eng.B == before
    # the per-step seam takes one scale
    class OwnStep(AEulerSampler):
        def step(self, x, fn, sigma, sigma_next, **kw):
            return super().step(x, fn, sigma, sigma_next, **kw)
    with pytest.raises(TypeError, match="needs the fused loop"):
        m.sample(seq, DEV, cond_scale=[1.0, 2.0, 7.5], timesteps=3, noise=torch.zeros(3, C, L, device=DEV), sampler=OwnStep())
    emb = m._embed(seq, DEV)
    with pytest.raises(TypeError, match="needs the fused loop"):
        m.diffusion.diffusion.denoise_fn(torch.zeros(3, C, L, device=DEV), sigma=torch.tensor(1.0), embedding=emb,
                                         embedding_scale=torch.tensor([1.0, 2.0, 7.5]))
    assert m.sample(seq, DEV, cond_scale=2.0, timesteps=3, noise=torch.zeros(3, C, L, device=DEV), sampler=OwnStep()).shape == (3, C, L)
