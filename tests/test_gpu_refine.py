"""-m gpu: refine() / refine_tokens() -- noise a lead up to the level of step k and run the remaining sampler steps, k per sample
(run_refine on mdt_refine_enter) -- against fixtures recorded from the real reference, the entry kernel against an independent host
reference, per-sample rows against their scalar calls bit for bit, known answers, an oracle loop at a batch no fixture has, the
strength sweep against its scalar calls and the custom op against the loop.

Tolerance: 1e-4 max-abs on the sample, as every parity test.  Tokens: the fixture generator asserts that every position of every case
has a top-two margin above 2e-4 in the reference, so tokens are compared at EVERY position.
"""
import os

import pytest
import torch

import refine_ref
from conftest import load_golden
from gpu_util import DEV, make_model
from helpers import oracle_cfg, synth_sd, to_t
from test_gpu_elem import NOISE_TOL
from moleculediffusiontransformer_amd import (ADPM2Sampler, AEulerSampler, KarrasSampler, KarrasSchedule, NoiseSource, one_hot_draft,
                                              ops, runtime as rt, strength_sweep)
from moleculediffusiontransformer_amd.synth import synth_normal
from oracle import unet_oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-4
SAMPLERS = {"adpm2": lambda: None, "aeuler": AEulerSampler}


@pytest.fixture(scope="module", params=["bf16x3", "f32", "f32-layers"])
def models(request):
    """The three product-mode forms of test_gpu_inpaint_tokens.py: split-bf16 MFMA, exact fp32 MFMA on the fused program, and the
    exact mode's layer-by-layer form."""
    cache = {}
    mode, _, form = request.param.partition("-")
    old = os.environ.get("MDT_F32_FUSED")
    os.environ["MDT_F32_FUSED"] = "0" if form == "layers" else "1"      # read when an engine is compiled

    def get(case):
        if case not in cache:
            cache[case] = make_model(case)
            cache[case].gemm_mode = mode
        return cache[case]
    get.mode = mode
    yield get
    if old is None:
        del os.environ["MDT_F32_FUSED"]
    else:
        os.environ["MDT_F32_FUSED"] = old


@pytest.fixture(scope="module")
def pinned():
    """tiny and pd22 in the default mode with the kernel choice pinned, for the bit-for-bit comparisons between calls."""
    cache = {}

    def get(case):
        if case not in cache:
            cache[case] = make_model(case)
            cache[case].kernel_choice = "narrow"
        return cache[case]
    return get


def fixture_cases():
    g = load_golden("refine.npz")
    return [(str(n), str(m), str(s), str(t)) for n, m, s, t in zip(g["cases"], g["models"], g["samplers"], g["tags"])]


def named_noise(tag, shape):
    """The draws of the fixture: draw 0 = the entry noise, draw i + 1 = step i, whatever the start."""
    return NoiseSource(init=synth_normal(f"{tag}/draw0", shape), steps=lambda i: synth_normal(f"{tag}/draw{i + 1}", shape))


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same(a, b):
    return torch.equal(bits(a), bits(b))


# ----------------------------------------------------------------------------------------------------------------------
# 1. the fixture of the real reference
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,model,sampler,tag", fixture_cases())
def test_fixture_parity(models, name, model, sampler, tag):
    g = {k[len(name) + 1:]: v for k, v in load_golden("refine.npz").items() if k.startswith(f"{name}_")}
    m = models(model)
    draft, out_ref, start = to_t(g["draft"]), to_t(g["out"]), g["start"].tolist()
    shape, T, cs = tuple(out_ref.shape), int(g["timesteps"]), float(g["cond_scale"])
    tok, out = m.refine_tokens(to_t(g["seq"]), DEV, draft, start, cond_scale=cs, timesteps=T, noise=named_noise(tag, shape),
                               sampler=SAMPLERS[sampler](), return_sample=True)
    assert tok.dtype == torch.int64 and tok.device.type == "cuda" and tok.shape == draft.shape
    assert out.dtype == torch.float32 and out.shape == shape
    err = float((out.cpu() - out_ref).abs().max())
    wrong = int((tok.cpu() != to_t(g["tokens"])).sum())
    print(f"refine_tokens {name} [{models.mode}]: max|hip - reference| = {err:.3e}, tokens differing = {wrong} of {tok.numel()}")
    assert err < TOL
    assert wrong == 0
    # the dense refine() on the one-hot draft with the same draws: the same loop, the same bits
    dense = m.refine(to_t(g["seq"]), DEV, one_hot_draft(draft, shape[1]), start, cond_scale=cs, timesteps=T,
                     noise=named_noise(tag, shape), sampler=SAMPLERS[sampler]())
    assert same(dense, out)


# ----------------------------------------------------------------------------------------------------------------------
# 2. the entry kernel against the host reference (refine_ref.py)
# ----------------------------------------------------------------------------------------------------------------------
# the last three are EDGE_SHAPES of test_gpu_elem.py: C = 1 at L = 4; odd C with Cp no power of two; L / 4 one past a wave
@pytest.mark.parametrize("B,C,L,Cp", [(5, 22, 32, 32), (3, 16, 64, 16), (3, 1, 4, 16), (2, 33, 36, 48), (2, 7, 260, 16)])
def test_entry_kernel_against_the_host_reference(B, C, L, Cp):
    """Explicit noise: float32 arithmetic in the kernel's order, bit for bit (sigma 2.75).  Seeded: against the float64 normals of
    noise_ref at NOISE_TOL, the bound of mdt_init_noise -- with sigma 0.5 the product is exact, the generator's deviation is halved
    (<= 1e-6) and the one rounding of the sum at |x| < 16 adds at most 4.8e-7, so the bound holds for x, and for xin = 0.36 x."""
    lib = rt.load_library()
    gen = torch.Generator().manual_seed(200 + C)
    x0, xin0 = torch.randn(B, C, L, generator=gen), torch.randn(B, L, Cp, generator=gen) + 3.0          # the pre-filled patterns
    dense = torch.randn(B, C, L, generator=gen)
    draft = torch.randint(0, C, (B, L), generator=gen).to(torch.int32)
    nz = torch.randn(B, C, L, generator=gen)
    i, c_in, seed, draw, sample0 = 3, 0.36, 0x1234567890, 3, 6
    starts = {"mixed": [i, i + 1, i, 0, i][:B], "none": [i + 1] * B, "all": [i] * B}
    g = lambda t: None if t is None else t.to(DEV)               # noqa: E731
    with torch.cuda.device(DEV):
        st = rt.current_stream()
        for which, start in starts.items():
            for form in ("dense", "token"):
                src, ids = (dense, None) if form == "dense" else (None, draft)
                for explicit in (True, False):
                    sigma = 2.75 if explicit else 0.5
                    what = (which, form, explicit)
                    gx, gxin, gs, gsrc, gids, gnz = g(x0), g(xin0), g(torch.tensor(start, dtype=torch.int32)), g(src), g(ids), g(nz)
                    rt.check(lib.mdt_refine_enter(rt.ptr(gx), rt.ptr(gxin), rt.ptr(gs), i, rt.ptr(gsrc), rt.ptr(gids),
                                                  rt.ptr(gnz) if explicit else 0, sigma, c_in, seed, draw, sample0, B, C, L, Cp, st))
                    torch.cuda.synchronize()
                    wx, wxin, entering = refine_ref.refine_enter(
                        x0.numpy(), xin0.numpy(), start, i, sigma, c_in, src=None if src is None else src.numpy(),
                        draft=None if ids is None else ids.numpy(), noise=nz.numpy() if explicit else None, seed=seed, draw=draw,
                        sample0=sample0)
                    assert entering.tolist() == [s == i for s in start], what
                    stay = torch.from_numpy(~entering)
                    # a row that does not enter is written neither in x nor in xin
                    assert same(gx.cpu()[stay], x0[stay]) and same(gxin.cpu()[stay], xin0[stay]), what
                    ent = torch.from_numpy(entering)
                    if not entering.any():
                        continue
                    assert bool((gxin.cpu()[ent][:, :, C:] == 0).all()), what                      # the pad columns
                    if explicit:
                        assert same(gx.cpu()[ent], torch.from_numpy(wx)[ent]), what
                        assert same(gxin.cpu()[ent], torch.from_numpy(wxin)[ent]), what
                    else:
                        dx = float((gx.cpu().double()[ent] - torch.from_numpy(wx)[ent]).abs().max())
                        dxin = float((gxin.cpu().double()[ent] - torch.from_numpy(wxin)[ent]).abs().max())
                        print(f"refine_enter {what}: max|x - host| = {dx:.3e}, max|xin - host| = {dxin:.3e}")
                        assert dx <= NOISE_TOL and dxin <= NOISE_TOL, what


# ----------------------------------------------------------------------------------------------------------------------
# 3. row b of a per-sample call is row b of the scalar call at start[b], bit for bit
# ----------------------------------------------------------------------------------------------------------------------
def stitched(call, starts):
    rows = call(starts)
    runs = {k: call(k) for k in sorted(set(starts))}
    return rows, tuple(torch.stack([runs[k][j][b] for b, k in enumerate(starts)]) for j in range(len(rows)))


@pytest.mark.parametrize("kind", ["adpm2", "aeuler", "karras40"])
def test_rows_equal_the_scalar_calls(pinned, kind):
    m = pinned("pd22")
    B, T, starts = 4, 6, [3, 0, 4, 1]
    make = {"adpm2": lambda: None, "aeuler": AEulerSampler, "karras40": lambda: KarrasSampler(s_churn=40)}[kind]
    seq = synth_normal("rf_rows/seq", (B, 12))
    draft = torch.randint(0, m.pred_dim, (B, m.max_length), generator=torch.Generator().manual_seed(71))
    for cs in (1.0, 2.0, torch.tensor([2.0, 1.0, 7.5, 2.0])):
        (tok, x), (tok_w, x_w) = stitched(lambda k: m.refine_tokens(seq, DEV, draft, k, cond_scale=cs, timesteps=T, sampler=make(),
                                                                    noise=NoiseSource(seed=41, sample0=5), return_sample=True), starts)
        assert bool(torch.isfinite(x).all()) and same(x, x_w) and torch.equal(tok, tok_w), (kind, cs)
        assert torch.equal(tok, x.argmax(dim=1))
    assert not same(x[0], x[2])
    # dynamic thresholding in force (sigma_data 1: the quantile passes 1, as in test_gpu_guidance_rows.py)
    kd = m.diffusion.diffusion
    sigma_data = kd.sigma_data
    kd.sigma_data, kd.dynamic_threshold = 1.0, 0.9
    try:
        (tok, x), (tok_w, x_w) = stitched(lambda k: m.refine_tokens(seq, DEV, draft, k, cond_scale=2.0, timesteps=T, sampler=make(),
                                                                    noise=NoiseSource(seed=41, sample0=5), return_sample=True), starts)
        assert bool(torch.isfinite(x).all()) and same(x, x_w) and torch.equal(tok, tok_w), kind
        kd.dynamic_threshold = 0.0
        plain = m.refine_tokens(seq, DEV, draft, starts, cond_scale=2.0, timesteps=T, sampler=make(),
                                noise=NoiseSource(seed=41, sample0=5), return_sample=True)[1]
    finally:
        kd.sigma_data, kd.dynamic_threshold = sigma_data, 0.0
    assert not same(plain, x)                                               # (the threshold was in force)
    assert m._engine.handoff_status() == 0


# ----------------------------------------------------------------------------------------------------------------------
# 4. known answers
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cs", [1.0, 2.0])
def test_zero_source_at_start_zero_is_sample(pinned, cs):
    m = pinned("tiny")
    B, C, L, T = 3, m.pred_dim, m.max_length, 6
    seq = synth_normal("tiny/seq", (B, 12))
    zeros = torch.zeros(B, C, L)
    for make in (lambda: None, AEulerSampler, lambda: KarrasSampler(s_churn=40)):
        for ns in (lambda: named_noise("rf_known", (B, C, L)), lambda: NoiseSource(seed=43, sample0=2)):
            want = m.sample(seq, DEV, cond_scale=cs, timesteps=T, noise=ns(), sampler=make())
            got = m.refine(seq, DEV, zeros, 0, cond_scale=cs, timesteps=T, noise=ns(), sampler=make())
            assert torch.equal(got, want) and bool(torch.isfinite(got).all())
    # clamp and trace carry over
    tr_a, tr_b = {"want": (1, T - 1)}, {"want": (1, T - 1)}
    want = m.sample(seq, DEV, cond_scale=cs, timesteps=T, clamp=True, noise=NoiseSource(seed=43), trace=tr_a)
    got = m.refine(seq, DEV, zeros, 0, cond_scale=cs, timesteps=T, clamp=True, noise=NoiseSource(seed=43), trace=tr_b)
    assert torch.equal(got, want) and float(got.abs().max()) <= 1.0
    assert torch.equal(tr_a[1], tr_b[1]) and torch.equal(tr_a[T - 1], tr_b[T - 1])


def test_karras_without_churn_returns_the_noised_source(pinned):
    """The reference's correction line (diffusion.py:434) does not move without churn: KarrasSampler() returns its starting state,
    src + sigmas[k] * draw0, bit for bit (a float32 multiply, then a float32 add)."""
    m = pinned("pd22")
    B, C, L, T = 3, m.pred_dim, m.max_length, 8
    seq = synth_normal("tiny/seq", (B, 12))
    src, draw0 = synth_normal("rf_k0/src", (B, C, L)), synth_normal("rf_k0/draw0", (B, C, L))
    sig = KarrasSchedule(0.001, 9.0, 3.0)(T)
    starts = [0, 3, T - 2]
    out = m.refine(seq, DEV, src, starts, cond_scale=1.0, timesteps=T, noise=draw0, sampler=KarrasSampler())
    want = torch.stack([src[b] + sig[k] * draw0[b] for b, k in enumerate(starts)])
    assert same(out, want)


def test_last_start_keeps_the_draft(models):
    """At start_step = T - 2 the lead is noised at sigmas[T - 2] ~ 3e-3 only: the reference keeps all 96 tokens of the fixture's
    draft, with a top-two margin of 2.0 (tests/golden/refine.npz, last_start_margin)."""
    g = load_golden("refine.npz")
    m = models("tiny")
    draft, T = to_t(g["a_draft"]), 8
    tok = m.refine_tokens(to_t(g["a_seq"]), DEV, draft, T - 2, cond_scale=1.0, timesteps=T, noise=named_noise("rf_tiny", (3, 16, 32)))
    assert torch.equal(tok.cpu(), draft)
    assert torch.equal(m.refine_tokens(to_t(g["a_seq"]), DEV, draft, strength=1e-9, cond_scale=1.0, timesteps=T,
                                       noise=named_noise("rf_tiny", (3, 16, 32))), tok)


# ----------------------------------------------------------------------------------------------------------------------
# 5. against a loop built from the oracle's public pieces, at a batch no fixture has
# ----------------------------------------------------------------------------------------------------------------------
def oracle_refine(sd, cfg, src, emb, T, k, draw0, step_noise, cs):
    """x = src + sigmas[k] * draw0, then ADPM2Sampler.step (diffusion.py:502-515) for i = k .. T - 2."""
    with torch.no_grad():
        sigmas = O.karras_sigmas(T)
        x = src + sigmas[k] * draw0
        for i in range(k, T - 1):
            sigma, sigma_next = sigmas[i], sigmas[i + 1]
            sigma_up, sigma_down, sigma_mid = O.adpm2_sigmas(sigma, sigma_next)
            d = (x - O.denoise(sd, cfg, x, sigma, emb, cs)) / sigma
            x_mid = x + d * (sigma_mid - sigma)
            d_mid = (x_mid - O.denoise(sd, cfg, x_mid, sigma_mid, emb, cs)) / sigma_mid
            x = x + d_mid * (sigma_down - sigma)
            x = x + step_noise(i) * sigma_up
        return x


def test_mixed_starts_against_the_oracle(models):
    m = models("tiny")
    B, C, L, T, cs = 5, 16, 32, 7, 2.0
    starts = [2, 0, 5, 3, 2]
    seq = synth_normal("rf_b5/seq", (B, 12))
    draft = torch.randint(0, C, (B, L), generator=torch.Generator().manual_seed(81))
    src = one_hot_draft(draft, C)
    sd, cfg = synth_sd("tiny"), oracle_cfg("tiny")
    ns = named_noise("rf_b5", (B, C, L))
    with torch.no_grad():
        emb = O.cond_embed(sd, cfg, seq)
    ref = torch.empty(B, C, L)
    for k in sorted(set(starts)):
        rows = [b for b, s in enumerate(starts) if s == k]
        ref[rows] = oracle_refine(sd, cfg, src[rows], emb[rows], T, k, ns.init[rows], lambda i: ns.steps(i)[rows], cs)
    tok, x = m.refine_tokens(seq, DEV, draft, starts, cond_scale=cs, timesteps=T, noise=named_noise("rf_b5", (B, C, L)),
                             return_sample=True)
    err = float((x.cpu() - ref).abs().max())
    print(f"refine_tokens B=5 starts {starts} [{models.mode}]: max|hip - oracle| = {err:.3e}")
    assert err < TOL
    top2 = torch.topk(ref, 2, dim=1).values
    sure = (top2[:, 0] - top2[:, 1]) > 2 * TOL                  # where the oracle's margin exceeds twice the sample tolerance
    assert torch.equal(tok.cpu()[sure], ref.argmax(dim=1)[sure])


# ----------------------------------------------------------------------------------------------------------------------
# 6. the sweep, 7. the op
# ----------------------------------------------------------------------------------------------------------------------
def test_strength_sweep_equals_the_scalar_calls(pinned):
    m = pinned("pd22")
    S, B, T = 3, 2, 8
    strengths = [0.25, 1.0, 0.5]
    seq = synth_normal("rf_sweep/seq", (B, 12))
    draft = torch.randint(0, m.pred_dim, (B, m.max_length), generator=torch.Generator().manual_seed(91))
    tok, x = strength_sweep(m, seq, draft, strengths, DEV, timesteps=T, cond_scale=2.0, noise=NoiseSource(seed=51, sample0=3),
                            return_sample=True)
    assert tok.shape == (S, B, m.max_length) and x.shape == (S, B, m.pred_dim, m.max_length) and torch.equal(tok, x.argmax(dim=2))
    for s, strength in enumerate(strengths):
        t_w, x_w = m.refine_tokens(seq, DEV, draft, strength=strength, timesteps=T, cond_scale=2.0,
                                   noise=NoiseSource(seed=51, sample0=3 + s * B), return_sample=True)
        assert same(x[s], x_w) and torch.equal(tok[s], t_w), s
    assert torch.equal(strength_sweep(m, seq, draft, strengths, DEV, timesteps=T, cond_scale=2.0, noise=NoiseSource(seed=51, sample0=3)),
                       tok)


def test_plain_call_is_the_single_op(pinned, monkeypatch):
    m = pinned("tiny")
    B, C, L, T = 3, m.pred_dim, m.max_length, 6
    seq = synth_normal("tiny/seq", (B, 12))
    draft = torch.randint(0, C, (B, L), generator=torch.Generator().manual_seed(95))
    from moleculediffusiontransformer_amd import generative as G
    calls = {"op": [], "direct": 0}
    loop = ops.run_refine

    def through_op(*a, **k):                           # the loop as the op's body calls it
        calls["op"].append(a[8])
        return loop(*a, **k)

    def direct(*a, **k):                               # the loop as refine() / refine_tokens() call it without the op
        calls["direct"] += 1
        return loop(*a, **k)
    monkeypatch.setattr(ops, "run_refine", through_op)
    monkeypatch.setattr(G, "run_refine", direct)
    for start in (2, [1, 4, 2]):
        for make in (lambda: None, AEulerSampler):
            calls["op"].clear()
            tok, x = m.refine_tokens(seq, DEV, draft, start, cond_scale=2.0, timesteps=T, noise=NoiseSource(seed=61, sample0=1),
                                     sampler=make(), return_sample=True)
            assert calls["direct"] == 0 and len(calls["op"]) == 1
            assert calls["op"][0].dtype == torch.int32 and calls["op"][0].tolist() == ([start] * B if isinstance(start, int) else start)
            # ... and equals run_refine called directly
            emb = m._embed(seq, DEV)
            eng = m.engine(DEV, emb.shape[1], 2 * B)
            tok_d = torch.zeros(B, L, dtype=torch.int32, device=DEV)
            with torch.no_grad():
                x_d = loop(eng, emb, C, T, NoiseSource(seed=61, sample0=1), KarrasSchedule(0.001, 9.0, 3.0),
                                 make() or ADPM2Sampler(rho=1), 0.1, start, draft=draft.to(DEV), embedding_scale=2.0, tokens=tok_d)
            assert same(x, x_d) and torch.equal(tok, tok_d.long())
    # the route with explicit step draws is not the op
    calls["op"].clear()
    tok_e = m.refine_tokens(seq, DEV, draft, 2, cond_scale=2.0, timesteps=T, noise=named_noise("rf_op", (B, C, L)))
    assert calls["op"] == [] and calls["direct"] == 1 and tok_e.shape == (B, L)
    # the op refuses what the loop refuses, as a RuntimeError
    emb = m._embed(seq, DEV)
    h = ops.register_engine(m.engine(DEV, emb.shape[1], 2 * B))
    sig = KarrasSchedule(0.001, 9.0, 3.0)(T)
    with pytest.raises(RuntimeError, match="start"):
        torch.ops.mdt.refine_tokens(emb, draft.to(DEV), torch.full((B,), T - 1, dtype=torch.int32, device=DEV), None, sig, h, C, 0,
                                    [1.0], 0.1, 1.0, 7, 0, 0.0)
    with pytest.raises(RuntimeError, match="int32"):
        torch.ops.mdt.refine_tokens(emb, draft.to(DEV), torch.zeros(B, dtype=torch.int64, device=DEV), None, sig, h, C, 0, [1.0], 0.1,
                                    1.0, 7, 0, 0.0)
