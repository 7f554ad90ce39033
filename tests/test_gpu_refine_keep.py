"""-m gpu: refine_keep(keep_mask=) / refine_keep_tokens(keep_mask=) -- refine a lead around a kept scaffold, k per sample (run_refine on
mdt_refine_keep_enter and mdt_inpaint_finish) -- the entry kernel against an independent host reference bit for bit, the fixture
recorded from the real reference, the identities with the unmasked call (nothing kept), with the source (everything kept) and with
the reference-pinned inpaint path (start 0, ADPM2), per-sample rows against their scalar calls, shards against the whole batch, the
custom op against the loop and the strength sweep against its scalar calls.

Tolerance: 1e-4 max-abs on the sample, as every parity test.  Tokens: the fixture generator asserts that every position of every case
has a top-two margin above 2e-4 in the reference, so tokens are compared at EVERY position.
"""
import pytest
import torch

import refine_keep_ref
from conftest import load_golden
from gpu_util import DEV
from helpers import to_t
from test_gpu_elem import NOISE_TOL
from test_gpu_refine import models, pinned, same, stitched  # noqa: F401  (models and pinned are fixtures)
from moleculediffusiontransformer_amd import (ADPM2Sampler, AEulerSampler, KarrasSampler, KarrasSchedule, NoiseSource, one_hot_draft,
                                              ops, runtime as rt, strength_sweep)
from moleculediffusiontransformer_amd.distributed import refine_keep_tokens_sharded
from moleculediffusiontransformer_amd.synth import synth_normal

pytestmark = pytest.mark.gpu
TOL = 1e-4
SAMPLERS = {"adpm2": lambda: None, "aeuler": AEulerSampler, "karras40": lambda: KarrasSampler(s_churn=40)}


def named_noise(tag, shape, T):
    """The draws of the fixture: draw 0 = the entry noise, draw i + 1 = step i, draw T + i = the source draw of step i."""
    return NoiseSource(init=synth_normal(f"{tag}/draw0", shape), steps=lambda i: synth_normal(f"{tag}/draw{i + 1}", shape),
                       sources=lambda i: synth_normal(f"{tag}/draw{T + i}", shape))


def expand(keep, C):
    return keep.unsqueeze(1).expand(-1, C, -1).contiguous()


def some_mask(B, L, seed):
    """(B, L): row 0 changes inside every group of four, row 1 is aligned blocks, the rest is random."""
    keep = torch.rand(B, L, generator=torch.Generator().manual_seed(seed)) < 0.4
    keep[0] = torch.arange(L) % 3 == 0
    if B > 1:
        keep[1] = (torch.arange(L) // 4) % 2 == 0
    return keep


# ----------------------------------------------------------------------------------------------------------------------
# 1. the entry kernel against the host reference (refine_keep_ref.py), bit for bit
# ----------------------------------------------------------------------------------------------------------------------
def row_masks(B, C, L, shift, gen):
    """A per-token (B, L) and a dense (B, C, L) mask whose rows cycle through: changing inside every group of four, all True, all
    False, random, aligned groups of four (fully kept and fully free quads side by side)."""
    tok, full = torch.zeros(B, L, dtype=torch.bool), torch.zeros(B, C, L, dtype=torch.bool)
    for b in range(B):
        kind = ("mixed", "true", "false", "random", "blocks")[(b + shift) % 5]
        if kind == "mixed":
            tok[b] = torch.arange(L) % 3 == 0
            full[b] = (torch.arange(C * L).view(C, L) % 3) == 0
        elif kind == "true":
            tok[b], full[b] = True, True
        elif kind == "random":
            tok[b] = torch.rand(L, generator=gen) < 0.5
            full[b] = torch.rand(C, L, generator=gen) < 0.5
        elif kind == "blocks":
            tok[b] = (torch.arange(L) // 4) % 2 == 0
            full[b] = ((torch.arange(C * L).view(C, L) // 4) % 2) == 0
    return tok, full


# the shapes of the entry-kernel test of test_gpu_refine.py
@pytest.mark.parametrize("B,C,L,Cp", [(5, 22, 32, 32), (3, 16, 64, 16), (3, 1, 4, 16), (2, 33, 36, 48), (2, 7, 260, 16)])
def test_entry_kernel_against_the_host_reference(B, C, L, Cp):
    """One launch holds rows with start below, at and above step_i (B = 2: two launches between them).  Explicit noise: float32
    arithmetic in the kernel's order, bit for bit (sigma 2.75).  Generator noise, twice: bit for bit against the host reference fed
    the device's own draws at (seed, step_entry / step_src, sample0) -- mdt_init_noise with sigma0 = 1, which test_gpu_elem.py pins to
    noise_ref -- and against the float64 normals of noise_ref at NOISE_TOL, the bound of mdt_init_noise: with sigma 0.5 the product is
    exact, the generator's deviation is halved (<= 1e-6) and the one rounding of the sum at |x| < 16 adds at most 4.8e-7, so the
    bound holds for x, and for xin = 0.36 x."""
    lib = rt.load_library()
    gen = torch.Generator().manual_seed(300 + C)
    x0, xin0 = torch.randn(B, C, L, generator=gen), torch.randn(B, L, Cp, generator=gen) + 3.0          # the pre-filled patterns
    dense = torch.randn(B, C, L, generator=gen)
    draft = torch.randint(0, C, (B, L), generator=gen).to(torch.int32)
    ne, ns = torch.randn(B, C, L, generator=gen), torch.randn(B, C, L, generator=gen)
    i, c_in, seed, d_entry, d_src, sample0 = 3, 0.36, 0x1234567890, 0, 11, 6
    g = lambda t: None if t is None else t.to(DEV)               # noqa: E731
    with torch.cuda.device(DEV):
        st = rt.current_stream()
        dev_draws = []
        for d in (d_entry, d_src):                               # the device's own draws, for the bit-for-bit generator leg
            z = torch.empty(B, C, L, device=DEV)
            rt.check(lib.mdt_init_noise(rt.ptr(z), 0, 1.0, seed, d, sample0, B, C, L, st))
            dev_draws.append(z)
        torch.cuda.synchronize()
        ze, zs = (z.cpu() for z in dev_draws)
        for start, shift in (([i - 2, i, i + 1, i, 0][:B], 0), ([i + 1, i - 1, i, i + 2, i][:B], 2)):
            tok_mask, full_mask = row_masks(B, C, L, shift, gen)
            for form in ("dense", "token"):
                src, ids = (dense, None) if form == "dense" else (None, draft)
                for per_token in (0, 1):
                    keep = tok_mask if per_token else full_mask
                    for explicit in (True, False):
                        sigma = 2.75 if explicit else 0.5
                        what = (start, form, per_token, explicit)
                        gx, gxin, gs = g(x0), g(xin0), g(torch.tensor(start, dtype=torch.int32))
                        gsrc, gids, gk, gne, gns = g(src), g(ids), g(keep.to(torch.uint8)), g(ne), g(ns)
                        rt.check(lib.mdt_refine_keep_enter(
                            rt.ptr(gx), rt.ptr(gxin), rt.ptr(gs), i, rt.ptr(gsrc), rt.ptr(gids), rt.ptr(gk), per_token,
                            rt.ptr(gne) if explicit else 0, rt.ptr(gns) if explicit else 0, sigma, c_in, seed, d_entry, d_src,
                            sample0, B, C, L, Cp, st))
                        torch.cuda.synchronize()
                        gx, gxin = gx.cpu(), gxin.cpu()
                        kw = dict(src=None if src is None else src.numpy(), draft=None if ids is None else ids.numpy())
                        n_e, n_s = (ne, ns) if explicit else (ze, zs)
                        wx, wxin, runs = refine_keep_ref.keep_enter(x0.numpy(), xin0.numpy(), start, i, sigma, c_in, keep.numpy(),
                                                                    n_entry=n_e.numpy(), n_src=n_s.numpy(), **kw)
                        assert runs.tolist() == [s <= i for s in start], what
                        wait = torch.from_numpy(~runs)
                        # a row that has not started keeps its sentinel in x and in xin
                        assert same(gx[wait], x0[wait]) and same(gxin[wait], xin0[wait]), what
                        run = torch.from_numpy(runs)
                        assert bool((gxin[run][:, :, C:] == 0).all()), what                        # the pad columns
                        assert same(gx[run], torch.from_numpy(wx)[run]), what
                        assert same(gxin[run], torch.from_numpy(wxin)[run]), what
                        if not explicit:                         # ... and against the independent float64 normals
                            hx, hxin, _ = refine_keep_ref.keep_enter(x0.numpy(), xin0.numpy(), start, i, sigma, c_in, keep.numpy(),
                                                                     seed=seed, draw_entry=d_entry, draw_src=d_src, sample0=sample0, **kw)
                            dx = float((gx.double()[run] - torch.from_numpy(hx)[run]).abs().max())
                            dxin = float((gxin.double()[run] - torch.from_numpy(hxin)[run]).abs().max())
                            print(f"refine_keep_enter {what}: max|x - host| = {dx:.3e}, max|xin - host| = {dxin:.3e}")
                            assert dx <= NOISE_TOL and dxin <= NOISE_TOL, what


# ----------------------------------------------------------------------------------------------------------------------
# 2. the fixture of the real reference
# ----------------------------------------------------------------------------------------------------------------------
def fixture_cases():
    g = load_golden("refine_keep.npz")
    return [(str(n), str(m), str(s), str(t)) for n, m, s, t in zip(g["cases"], g["models"], g["samplers"], g["tags"])]


@pytest.mark.parametrize("name,model,sampler,tag", fixture_cases())
def test_fixture_parity(models, name, model, sampler, tag):  # noqa: F811
    g = {k[len(name) + 1:]: v for k, v in load_golden("refine_keep.npz").items() if k.startswith(f"{name}_")}
    m = models(model)
    draft, keep, out_ref, start = to_t(g["draft"]), to_t(g["keep"]), to_t(g["out"]), g["start"].tolist()
    shape, T, cs = tuple(out_ref.shape), int(g["timesteps"]), float(g["cond_scale"])
    tok, out = m.refine_keep_tokens(to_t(g["seq"]), DEV, draft, start, cond_scale=cs, timesteps=T, noise=named_noise(tag, shape, T),
                                    sampler=SAMPLERS[sampler](), return_sample=True, keep_mask=keep)
    assert tok.dtype == torch.int64 and tok.device.type == "cuda" and tok.shape == draft.shape
    assert out.dtype == torch.float32 and out.shape == shape
    err = float((out.cpu() - out_ref).abs().max())
    wrong = int((tok.cpu() != to_t(g["tokens"])).sum())
    print(f"refine_keep_tokens() {name} [{models.mode}]: max|hip - reference| = {err:.3e}, tokens differing = {wrong} of "
          f"{tok.numel()}")
    assert err < TOL
    assert wrong == 0
    # the dense refine() on the one-hot draft with the same draws, the mask per position and per element: the same bits
    for mask in (keep, expand(keep, shape[1])):
        dense = m.refine_keep(to_t(g["seq"]), DEV, one_hot_draft(draft, shape[1]), start, cond_scale=cs, timesteps=T,
                              noise=named_noise(tag, shape, T), sampler=SAMPLERS[sampler](), keep_mask=mask)
        assert same(dense, out)


# ----------------------------------------------------------------------------------------------------------------------
# 3. nothing kept: the unmasked call; 4. everything kept: the source
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(SAMPLERS))
def test_all_false_mask_is_the_unmasked_call(pinned, kind):  # noqa: F811
    m = pinned("pd22")
    B, C, L, T, starts = 3, m.pred_dim, m.max_length, 6, [2, 0, 4]
    seq = synth_normal("rk_none/seq", (B, 12))
    draft = torch.randint(0, C, (B, L), generator=torch.Generator().manual_seed(73))
    src = synth_normal("rk_none/src", (B, C, L))
    none = torch.zeros(B, L, dtype=torch.bool)
    for ns in (lambda: NoiseSource(seed=47, sample0=3), lambda: named_noise("rk_none", (B, C, L), T)):
        for start in (1, starts):
            tok_w, x_w = m.refine_tokens(seq, DEV, draft, start, cond_scale=2.0, timesteps=T, noise=ns(), sampler=SAMPLERS[kind](),
                                         return_sample=True)
            tok, x = m.refine_keep_tokens(seq, DEV, draft, start, cond_scale=2.0, timesteps=T, noise=ns(), sampler=SAMPLERS[kind](),
                                          return_sample=True, keep_mask=none)
            assert bool(torch.isfinite(x).all()) and same(x, x_w) and torch.equal(tok, tok_w), (kind, start)
            want = m.refine(seq, DEV, src, start, cond_scale=2.0, timesteps=T, noise=ns(), sampler=SAMPLERS[kind](), clamp=True)
            for mask in (none, expand(none, C)):
                got = m.refine_keep(seq, DEV, src, start, cond_scale=2.0, timesteps=T, noise=ns(), sampler=SAMPLERS[kind](), clamp=True,
                                    keep_mask=mask)
                assert same(got, want), (kind, start)


@pytest.mark.parametrize("kind", list(SAMPLERS))
def test_all_true_mask_returns_the_source(pinned, kind):  # noqa: F811
    m = pinned("tiny")
    B, C, L, T = 3, m.pred_dim, m.max_length, 6
    seq = synth_normal("rk_all/seq", (B, 12))
    draft = torch.randint(0, C, (B, L), generator=torch.Generator().manual_seed(75))
    src = synth_normal("rk_all/src", (B, C, L))
    every = torch.ones(B, L, dtype=torch.bool)
    for start in (0, T - 2, [0, 3, T - 2]):
        tok, x = m.refine_keep_tokens(seq, DEV, draft, start, cond_scale=2.0, timesteps=T, noise=NoiseSource(seed=49),
                                      sampler=SAMPLERS[kind](), return_sample=True, keep_mask=every)
        assert torch.equal(tok.cpu(), draft) and same(x, one_hot_draft(draft, C)), (kind, start)
        for mask in (every, expand(every, C)):
            got = m.refine_keep(seq, DEV, src, start, cond_scale=1.0, timesteps=T, noise=NoiseSource(seed=49), sampler=SAMPLERS[kind](),
                                keep_mask=mask)
            assert same(got, src), (kind, start)


# ----------------------------------------------------------------------------------------------------------------------
# 5. start 0 under ADPM2 is the reference-pinned inpaint path
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cs", [1.0, 2.0])
def test_start_zero_adpm2_is_inpaint(pinned, cs):  # noqa: F811
    """refine(source * mask, start_step=0, keep_mask=mask) and inpaint(source, mask, num_resamples=1) on the same tensors: the free
    positions start as 0 + sigmas[0] * draw0 -- inpaint's sigmas[0] * draw0 up to the sign of a zero, hence torch.equal, not bits."""
    m = pinned("pd22")
    B, C, L, T = 3, m.pred_dim, m.max_length, 6
    seq = synth_normal("rk_inp/seq", (B, 12))
    source = synth_normal("rk_inp/src", (B, C, L))
    mask = torch.rand(B, C, L, generator=torch.Generator().manual_seed(77)) < 0.5
    mask[0, :, ::3] = True
    init = synth_normal("rk_inp/init", (B, C, L))
    steps = lambda i: synth_normal(f"rk_inp/step{i}", (B, C, L))       # noqa: E731
    sources = lambda i: synth_normal(f"rk_inp/source{i}", (B, C, L))   # noqa: E731
    order = [init] + [t for i in range(T - 1) for t in (sources(i), steps(i))]     # inpaint's call order (diffusion.py:535-547)
    it = iter(order)
    want = m.inpaint(seq, DEV, cond_scale=cs, timesteps=T, num_resamples=1, inpaint=source.to(DEV), in_paint_mask=mask.to(DEV),
                     draw=lambda like=None: next(it))
    assert next(it, None) is None                                      # every tensor was drawn
    got = m.refine_keep(seq, DEV, source * mask, 0, cond_scale=cs, timesteps=T,
                        noise=NoiseSource(init=init, steps=steps, sources=sources), keep_mask=mask)
    assert bool(torch.isfinite(got).all()) and torch.equal(got, want)
    assert same(got.cpu()[mask], source[mask])


# ----------------------------------------------------------------------------------------------------------------------
# 6. row b of a per-sample call is row b of the scalar call at start[b], bit for bit; 7. the kept positions
# ----------------------------------------------------------------------------------------------------------------------
def kept_exactly(tok, x, draft, keep):
    C = x.shape[1]
    full = expand(keep, C)
    return torch.equal(tok.cpu()[keep], draft[keep]) and same(x.cpu()[full], one_hot_draft(draft, C)[full])


@pytest.mark.parametrize("kind", list(SAMPLERS))
def test_rows_equal_the_scalar_calls_and_kept_positions_stay(pinned, kind):  # noqa: F811
    m = pinned("pd22")
    B, T, starts = 4, 6, [3, 0, 4, 1]
    seq = synth_normal("rk_rows/seq", (B, 12))
    draft = torch.randint(0, m.pred_dim, (B, m.max_length), generator=torch.Generator().manual_seed(71))
    keep = some_mask(B, m.max_length, 72)
    scales = (2.0, torch.tensor([2.0, 1.0, 7.5, 2.0])) if kind == "adpm2" else (2.0,)
    call = lambda cs: (lambda k: m.refine_keep_tokens(seq, DEV, draft, k, cond_scale=cs, timesteps=T,   # noqa: E731
                                                      sampler=SAMPLERS[kind](), noise=NoiseSource(seed=41, sample0=5),
                                                      return_sample=True, keep_mask=keep))
    for cs in scales:
        (tok, x), (tok_w, x_w) = stitched(call(cs), starts)
        assert bool(torch.isfinite(x).all()) and same(x, x_w) and torch.equal(tok, tok_w), (kind, cs)
        assert kept_exactly(tok, x, draft, keep), (kind, cs)
        assert torch.equal(tok.cpu()[~keep], x.cpu().argmax(dim=1)[~keep])
        if not isinstance(cs, torch.Tensor):
            free = m.refine_tokens(seq, DEV, draft, starts, cond_scale=cs, timesteps=T, sampler=SAMPLERS[kind](),
                                   noise=NoiseSource(seed=41, sample0=5), return_sample=True)[1]
            assert not same(free, x)                                        # (the mask was in force)
    assert not same(x[0], x[2])
    # dynamic thresholding in force (sigma_data 1: the quantile passes 1, as in test_gpu_guidance_rows.py)
    kd = m.diffusion.diffusion
    sigma_data = kd.sigma_data
    kd.sigma_data, kd.dynamic_threshold = 1.0, 0.9
    try:
        (tok, x), (tok_w, x_w) = stitched(call(2.0), starts)
        assert bool(torch.isfinite(x).all()) and same(x, x_w) and torch.equal(tok, tok_w), kind
        assert kept_exactly(tok, x, draft, keep), kind
        kd.dynamic_threshold = 0.0
        plain = call(2.0)(starts)[1]
    finally:
        kd.sigma_data, kd.dynamic_threshold = sigma_data, 0.0
    assert not same(plain, x)                                               # (the threshold was in force)
    assert m._engine.handoff_status() == 0


# ----------------------------------------------------------------------------------------------------------------------
# 8. shards, 9. the op, 10. the sweep
# ----------------------------------------------------------------------------------------------------------------------
def test_two_shards_equal_the_whole_batch(pinned):  # noqa: F811
    m = pinned("pd22")
    B, T, starts = 5, 6, [3, 0, 4, 1, 3]
    seq = synth_normal("rk_shard/seq", (B, 12))
    draft = torch.randint(0, m.pred_dim, (B, m.max_length), generator=torch.Generator().manual_seed(79))
    keep = some_mask(B, m.max_length, 80)

    def local(s, d, st, first, keep_mask):
        return m.refine_keep_tokens(s, DEV, d, st, cond_scale=2.0, timesteps=T, noise=NoiseSource(seed=53, sample0=7 + first),
                                    return_sample=True, keep_mask=keep_mask)
    tok, x = local(seq, draft, starts, 0, keep)
    parts = [local(seq[lo:hi], draft[lo:hi], starts[lo:hi], lo, keep[lo:hi]) for lo, hi in ((0, 3), (3, 5))]
    assert same(x, torch.cat([p[1] for p in parts])) and torch.equal(tok, torch.cat([p[0] for p in parts]))
    # the sharded wrapper, one rank: the local call on the whole batch
    got = refine_keep_tokens_sharded(lambda *a, **k: local(*a, **k)[0], seq, draft, starts, vocab=m.pred_dim, keep_mask=keep)
    assert torch.equal(got, tok)


def test_plain_masked_call_is_the_single_op(pinned, monkeypatch):  # noqa: F811
    m = pinned("tiny")
    B, C, L, T = 3, m.pred_dim, m.max_length, 6
    seq = synth_normal("tiny/seq", (B, 12))
    draft = torch.randint(0, C, (B, L), generator=torch.Generator().manual_seed(95))
    keep = some_mask(B, L, 96)
    from moleculediffusiontransformer_amd import generative as G
    calls = {"op": [], "direct": 0}
    loop = ops.run_refine

    def through_op(*a, **k):                           # the loop as the op's body calls it
        calls["op"].append(k)
        return loop(*a, **k)

    def direct(*a, **k):                               # the loop as refine() / refine_tokens() call it without the op
        calls["direct"] += 1
        return loop(*a, **k)
    monkeypatch.setattr(ops, "run_refine", through_op)
    monkeypatch.setattr(G, "run_refine", direct)
    for start in (2, [1, 4, 2]):
        for make in (lambda: None, AEulerSampler):
            calls["op"].clear()
            tok, x = m.refine_keep_tokens(seq, DEV, draft, start, cond_scale=2.0, timesteps=T, noise=NoiseSource(seed=61, sample0=1),
                                          sampler=make(), return_sample=True, keep_mask=keep)
            assert calls["direct"] == 0 and len(calls["op"]) == 1
            assert calls["op"][0]["keep_per_token"] is True and torch.equal(calls["op"][0]["keep"].cpu(), keep)
            # ... and equals run_refine called directly
            emb = m._embed(seq, DEV)
            eng = m.engine(DEV, emb.shape[1], 2 * B)
            tok_d = torch.zeros(B, L, dtype=torch.int32, device=DEV)
            with torch.no_grad():
                x_d = loop(eng, emb, C, T, NoiseSource(seed=61, sample0=1), KarrasSchedule(0.001, 9.0, 3.0),
                           make() or ADPM2Sampler(rho=1), 0.1, start, draft=draft.to(DEV), embedding_scale=2.0, tokens=tok_d,
                           keep=keep.to(DEV), keep_per_token=True)
            assert same(x, x_d) and torch.equal(tok, tok_d.long()) and kept_exactly(tok, x, draft, keep)
    # the route with explicit draws is not the op
    calls["op"].clear()
    tok_e = m.refine_keep_tokens(seq, DEV, draft, 2, cond_scale=2.0, timesteps=T, noise=named_noise("rk_op", (B, C, L), T),
                                 keep_mask=keep)
    assert calls["op"] == [] and calls["direct"] == 1 and tok_e.shape == (B, L)
    # the op refuses what the loop refuses, as a RuntimeError
    emb = m._embed(seq, DEV)
    h = ops.register_engine(m.engine(DEV, emb.shape[1], 2 * B))
    sig = KarrasSchedule(0.001, 9.0, 3.0)(T)
    start = torch.full((B,), 2, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="start"):
        torch.ops.mdt.refine_keep_tokens(emb, draft.to(DEV), start + T, keep.to(DEV), None, sig, h, C, 0, [1.0], 0.1, 1.0, 7, 0, 0.0)
    with pytest.raises(RuntimeError, match="keep"):
        torch.ops.mdt.refine_keep_tokens(emb, draft.to(DEV), start, keep.to(DEV).long(), None, sig, h, C, 0, [1.0], 0.1, 1.0, 7, 0, 0.0)


def test_strength_sweep_with_a_mask_equals_the_scalar_calls(pinned):  # noqa: F811
    m = pinned("pd22")
    S, B, T = 3, 2, 8
    strengths = [0.25, 1.0, 0.5]
    seq = synth_normal("rk_sweep/seq", (B, 12))
    draft = torch.randint(0, m.pred_dim, (B, m.max_length), generator=torch.Generator().manual_seed(91))
    keep = some_mask(B, m.max_length, 92)
    tok, x = strength_sweep(m, seq, draft, strengths, DEV, timesteps=T, cond_scale=2.0, noise=NoiseSource(seed=51, sample0=3),
                            return_sample=True, keep_mask=keep)
    assert tok.shape == (S, B, m.max_length) and x.shape == (S, B, m.pred_dim, m.max_length)
    for s, strength in enumerate(strengths):
        t_w, x_w = m.refine_keep_tokens(seq, DEV, draft, strength=strength, timesteps=T, cond_scale=2.0,
                                        noise=NoiseSource(seed=51, sample0=3 + s * B), return_sample=True, keep_mask=keep)
        assert same(x[s], x_w) and torch.equal(tok[s], t_w) and kept_exactly(tok[s], x[s], draft, keep), s
