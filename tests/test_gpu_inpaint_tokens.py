"""-m gpu: inpaint_tokens() -- draft completion from token ids on the fused inpainting loop (mdt_inpaint_enter / mdt_inpaint_finish)
-- against fixtures recorded from the real reference, against the dense inpaint() bit for bit, against the kernels it fuses bit for
bit, and against the oracle at a batch no fixture has.

Tolerance: 1e-4 max-abs on the sample, as every parity test.  Tokens: the fixture generator asserts that every generated position of
every case has a top-two margin above 2e-4 in the reference, so tokens are compared at EVERY position.
"""
import os

import pytest
import torch

from conftest import load_golden
from gpu_util import DEV, make_model
from helpers import oracle_cfg, synth_sd, to_t
from moleculediffusiontransformer_amd import one_hot_draft, runtime as rt
from moleculediffusiontransformer_amd.synth import synth_normal
from oracle import unet_oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-4


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
    get.mode = mode
    yield get
    if old is None:
        del os.environ["MDT_F32_FUSED"]
    else:
        os.environ["MDT_F32_FUSED"] = old


def fixture_cases():
    g = load_golden("inpaint_tokens.npz")
    return [(str(n), str(m), str(t)) for n, m, t in zip(g["cases"], g["models"], g["tags"])]


def named_draws(tag, shape):
    n = {"i": 0}

    def draw(like=None):
        t = synth_normal(f"{tag}/draw{n['i']}", shape)
        n["i"] += 1
        return t
    return draw, n


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def expand(keep, C):
    return keep.unsqueeze(1).expand(-1, C, -1).contiguous()


@pytest.mark.parametrize("name,model,tag", fixture_cases())
def test_fixture_parity(models, name, model, tag):
    g = {k[len(name) + 1:]: v for k, v in load_golden("inpaint_tokens.npz").items() if k.startswith(f"{name}_")}
    m = models(model)
    draft, keep, out_ref = to_t(g["draft"]), to_t(g["keep"]), to_t(g["out"])
    draw, n = named_draws(tag, tuple(out_ref.shape))
    tok, out = m.inpaint_tokens(to_t(g["seq"]), DEV, draft, keep, cond_scale=float(g["cond_scale"]), timesteps=int(g["timesteps"]),
                                num_resamples=int(g["num_resamples"]), draw=draw, return_sample=True)
    assert n["i"] == int(g["ndraws"])
    assert tok.dtype == torch.int64 and tok.device.type == "cuda" and tok.shape == draft.shape
    assert out.dtype == torch.float32 and out.shape == out_ref.shape
    err = float((out.cpu() - out_ref).abs().max())
    wrong = int((tok.cpu() != to_t(g["tokens"])).sum())
    print(f"inpaint_tokens {name} [{models.mode}]: max|hip - reference| = {err:.3e}, tokens differing = {wrong} of {tok.numel()}")
    assert err < TOL
    assert wrong == 0
    mask = expand(keep, out_ref.shape[1])
    assert torch.equal(bits(out)[mask], bits(one_hot_draft(draft, out_ref.shape[1]))[mask])
    # the dense inpaint() on the one-hot draft with the same draws: the same loop, the same bits
    draw, n = named_draws(tag, tuple(out_ref.shape))
    dense = m.inpaint(to_t(g["seq"]), DEV, cond_scale=float(g["cond_scale"]), timesteps=int(g["timesteps"]),
                      num_resamples=int(g["num_resamples"]), inpaint=one_hot_draft(draft, out_ref.shape[1]).to(DEV),
                      in_paint_mask=mask.to(DEV), draw=draw)
    assert n["i"] == int(g["ndraws"]) and torch.equal(bits(dense), bits(out))


@pytest.mark.parametrize("cond_scale", [1.0, 2.0])
@pytest.mark.parametrize("R", [1, 3])
def test_seed_mode_equals_dense_inpaint_bit_for_bit(models, cond_scale, R):
    m = models("pd22")
    B, C, L = 4, m.pred_dim, m.max_length
    seq = synth_normal("it_seed/seq", (B, 12))
    draft = torch.randint(0, C, (B, L), generator=torch.Generator().manual_seed(11))
    keep = torch.rand(B, L, generator=torch.Generator().manual_seed(12)) < 0.4
    tok, x = m.inpaint_tokens(seq, DEV, draft, keep, cond_scale=cond_scale, timesteps=5, num_resamples=R, seed=1234,
                              return_sample=True)
    dense = m.inpaint(seq, DEV, cond_scale=cond_scale, timesteps=5, num_resamples=R, inpaint=one_hot_draft(draft, C).to(DEV),
                      in_paint_mask=expand(keep, C).to(DEV), seed=1234)
    assert torch.equal(bits(x), bits(dense))
    tok, am = tok.cpu(), dense.argmax(dim=1).cpu()
    assert torch.equal(tok[~keep], am[~keep]) and torch.equal(tok[keep], draft[keep])
    assert torch.equal(m.inpaint_tokens(seq, DEV, draft, keep, cond_scale=cond_scale, timesteps=5, num_resamples=R, seed=1234).cpu(),
                       tok)
    other = m.inpaint_tokens(seq, DEV, draft, keep, cond_scale=cond_scale, timesteps=5, num_resamples=R, seed=1235,
                             return_sample=True)[1]
    assert not torch.equal(other, x)


# the last three are EDGE_SHAPES of test_gpu_elem.py: C = 1 at L = 4; odd C with Cp no power of two; L / 4 one past a wave
@pytest.mark.parametrize("B,C,L,Cp", [(5, 22, 32, 32), (3, 16, 64, 16), (3, 1, 4, 16), (2, 33, 36, 48), (2, 7, 260, 16)])
def test_enter_and_finish_kernels_equal_the_kernels_they_fuse_bit_for_bit(B, C, L, Cp):
    lib = rt.load_library()
    gen = torch.Generator().manual_seed(100 + C)
    x0 = torch.randn(B, C, L, generator=gen).to(DEV)
    dense_src = torch.randn(B, C, L, generator=gen).to(DEV)
    dense_keep = (torch.rand(B, C, L, generator=gen) < 0.5).to(torch.uint8).to(DEV)
    draft = torch.randint(0, C, (B, L), generator=gen).to(torch.int32).to(DEV)
    tok_keep = (torch.rand(B, L, generator=gen) < 0.5).to(torch.uint8)
    tok_keep[0], tok_keep[1] = 1, 0                       # an all-kept and a none-kept sample
    tok_keep = tok_keep.to(DEV)
    n_src, n_re = torch.randn(B, C, L, generator=gen).to(DEV), torch.randn(B, C, L, generator=gen).to(DEV)
    sigma, c_in, seed, k_src, k_re, sample0 = 2.75, 0.36, 0x1234567890, 3, 4, 6
    forms = {"dense": (dense_src, None, dense_keep, 0, dense_src, dense_keep),
             "token": (None, draft, tok_keep, 1, one_hot_draft(draft, C).to(DEV),
                       tok_keep.unsqueeze(1).expand(-1, C, -1).contiguous())}
    with torch.cuda.device(DEV):
        st = rt.current_stream()
        for form, (src, ids, keep, per_token, src_full, keep_full) in forms.items():
            for explicit in (True, False):
                for renoise in (0.0, 0.62):
                    ns, nr = (n_src, n_re) if explicit else (None, None)
                    xa = x0.clone()
                    if renoise:
                        rt.check(lib.mdt_add_noise(rt.ptr(xa), rt.ptr(nr), renoise, seed, k_re, sample0, B, C, L, st))
                    rt.check(lib.mdt_inpaint_merge(rt.ptr(xa), rt.ptr(src_full), rt.ptr(keep_full), rt.ptr(ns), sigma, seed, k_src,
                                                   sample0, B, C, L, st))
                    xin_a = torch.full((B, L, Cp), 7.0, device=DEV)
                    rt.check(lib.mdt_precond_in(rt.ptr(xa), rt.ptr(xin_a), c_in, B, C, L, Cp, st))
                    xb, xin_b = x0.clone(), torch.full((B, L, Cp), 9.0, device=DEV)
                    rt.check(lib.mdt_inpaint_enter(rt.ptr(xb), rt.ptr(xin_b), rt.ptr(src), rt.ptr(ids), rt.ptr(keep), per_token,
                                                   rt.ptr(ns), rt.ptr(nr), sigma, renoise, c_in, seed, k_src, k_re, sample0,
                                                   B, C, L, Cp, st))
                    what = (form, explicit, renoise)
                    assert torch.equal(bits(xa), bits(xb)), what
                    assert torch.equal(bits(xin_a), bits(xin_b)), what
                    assert not torch.equal(xb, x0) and bool((xin_b[:, :, C:] == 0).all()), what
            # the exit: merge at sigma 0 + decode (+ the draft id at a kept position of the token form)
            xa = x0.clone()
            rt.check(lib.mdt_inpaint_merge(rt.ptr(xa), rt.ptr(src_full), rt.ptr(keep_full), 0, 0.0, 0, 0, 0, B, C, L, st))
            tok_a = torch.zeros(B, L, dtype=torch.int32, device=DEV)
            rt.check(lib.mdt_argmax_tokens(rt.ptr(xa), rt.ptr(tok_a), B, C, L, st))
            if per_token:
                tok_a = torch.where(keep.bool(), draft, tok_a)
            xb, tok_b = x0.clone(), torch.full((B, L), -5, dtype=torch.int32, device=DEV)
            rt.check(lib.mdt_inpaint_finish(rt.ptr(xb), rt.ptr(src), rt.ptr(ids), rt.ptr(keep), per_token, rt.ptr(tok_b), B, C, L, st))
            assert torch.equal(bits(xa), bits(xb)) and torch.equal(tok_a, tok_b), form
            xc = x0.clone()                                # tokens == NULL: the merge alone
            rt.check(lib.mdt_inpaint_finish(rt.ptr(xc), rt.ptr(src), rt.ptr(ids), rt.ptr(keep), per_token, 0, B, C, L, st))
            assert torch.equal(bits(xc), bits(xb)), form
        # ties go to the first maximum, as mdt_argmax_tokens: a constant sample decodes to 0 at every generated position
        flat = torch.full((B, C, L), 0.25, device=DEV)
        tok = torch.full((B, L), -5, dtype=torch.int32, device=DEV)
        rt.check(lib.mdt_inpaint_finish(rt.ptr(flat), 0, rt.ptr(draft), rt.ptr(tok_keep), 1, rt.ptr(tok), B, C, L, st))
        assert torch.equal(tok, torch.where(tok_keep.bool(), draft, torch.zeros_like(draft)))
        torch.cuda.synchronize()


@pytest.mark.parametrize("cond_scale", [1.0, 2.0])
def test_shard_invariance(models, cond_scale):
    """Two half-batches with sample0 = 0 and B / 2 are the whole batch bit for bit, with the kernel choice pinned as the sharded
    wrappers pin it; inpaint(sample0=) likewise."""
    from moleculediffusiontransformer_amd.distributed import pin_for_shards
    m = models("tiny")
    B, C, L = 8, m.pred_dim, m.max_length
    seq = synth_normal("it_shard/seq", (B, 12))
    draft = torch.randint(0, C, (B, L), generator=torch.Generator().manual_seed(21))
    keep = torch.rand(B, L, generator=torch.Generator().manual_seed(22)) < 0.5
    pin_for_shards(m, B, 2, guided=cond_scale != 1.0)
    try:
        run = lambda lo, hi: m.inpaint_tokens(seq[lo:hi], DEV, draft[lo:hi], keep[lo:hi], cond_scale=cond_scale, timesteps=5,   # noqa: E731
                                              num_resamples=2, seed=99, sample0=lo, return_sample=True)
        tok, x = run(0, B)
        (t0, x0), (t1, x1) = run(0, B // 2), run(B // 2, B)
        assert torch.equal(bits(torch.cat([x0, x1])), bits(x)) and torch.equal(torch.cat([t0, t1]), tok)
        src, mask = one_hot_draft(draft, C).to(DEV), expand(keep, C).to(DEV)
        dense = lambda lo, hi: m.inpaint(seq[lo:hi], DEV, cond_scale=cond_scale, timesteps=5, num_resamples=2,                 # noqa: E731
                                         inpaint=src[lo:hi], in_paint_mask=mask[lo:hi], seed=99, sample0=lo)
        assert torch.equal(bits(torch.cat([dense(0, B // 2), dense(B // 2, B)])), bits(x))
    finally:
        m.pin_kernel_choice(None)


def test_all_kept_and_none_kept_rows(models):
    m = models("tiny")
    B, C, L = 3, m.pred_dim, m.max_length
    seq = synth_normal("it_rows/seq", (B, 12))
    draft = torch.randint(0, C, (B, L), generator=torch.Generator().manual_seed(31))
    keep = torch.zeros(B, L, dtype=torch.bool)
    keep[0] = True                                         # row 0: all kept; row 1: none kept; row 2: half
    keep[2, ::2] = True
    tok, x = m.inpaint_tokens(seq, DEV, draft, keep, cond_scale=2.0, timesteps=6, num_resamples=2, seed=5, return_sample=True)
    tok, x = tok.cpu(), x.cpu()
    assert torch.equal(tok[0], draft[0]) and torch.equal(bits(x[0]), bits(one_hot_draft(draft, C)[0]))
    assert bool(torch.isfinite(x).all()) and int(tok.min()) >= 0 and int(tok.max()) < C
    assert torch.equal(tok[1], x[1].argmax(dim=0)) and torch.equal(tok[2, ::2], draft[2, ::2])
    # an empty batch
    t0, x0 = m.inpaint_tokens(seq[:0], DEV, draft[:0], keep[:0], seed=5, return_sample=True)
    assert t0.shape == (0, L) and t0.dtype == torch.int64 and x0.shape == (0, C, L) and t0.device.type == "cuda"


def test_batch64_against_the_oracle(models):
    """The configs[1]-shaped model (c 64, pred_dim 16, L 64) at a batch no fixture has, explicit draws, under guidance."""
    m = models("cfg1")
    B, C, L, T, R, cs = 64, 16, 64, 4, 2, 2.0
    seq = synth_normal("it_b64/seq", (B, 12))
    draft = torch.randint(0, C, (B, L), generator=torch.Generator().manual_seed(41))
    keep = torch.rand(B, L, generator=torch.Generator().manual_seed(42)) < 0.5
    src, mask = one_hot_draft(draft, C), expand(keep, C)
    sd, cfg = synth_sd("cfg1"), oracle_cfg("cfg1")
    draw, n = named_draws("it_b64", (B, C, L))
    with torch.no_grad():
        emb = O.cond_embed(sd, cfg, seq)
    ref = O.adpm2_inpaint(sd, cfg, src, mask, emb, T, R, draw, cs)
    ndraws = n["i"]
    assert ndraws == 1 + (T - 1) * 2 * R
    draw, n = named_draws("it_b64", (B, C, L))
    tok, x = m.inpaint_tokens(seq, DEV, draft, keep, cond_scale=cs, timesteps=T, num_resamples=R, draw=draw, return_sample=True)
    assert n["i"] == ndraws
    err = float((x.cpu() - ref).abs().max())
    print(f"inpaint_tokens B=64 [{models.mode}]: max|hip - oracle| = {err:.3e}")
    assert err < TOL
    assert torch.equal(bits(x)[mask], bits(src)[mask]) and torch.equal(tok.cpu()[keep], draft[keep])
    top2 = torch.topk(ref, 2, dim=1).values
    sure = ((top2[:, 0] - top2[:, 1]) > 2 * TOL) & ~keep        # where the oracle's margin exceeds twice the sample tolerance
    assert torch.equal(tok.cpu()[sure], ref.argmax(dim=1)[sure])


def test_complete_and_validate_stays_on_the_device():
    """inpaint_from_draft_and_conditioning's core (generative.py:1600-1660): draft completion -> re-tokenise -> forward model."""
    from moleculediffusiontransformer_amd import NoiseSource, complete_and_validate, predict_properties_from_tokens
    inv, fwd = make_model("tiny"), make_model("cfg3")
    cond = synth_normal("it_chain/cond", (4, 12))
    draft = torch.randint(0, inv.pred_dim, (4, 32), generator=torch.Generator().manual_seed(51))
    keep = torch.zeros(4, 32, dtype=torch.bool)
    keep[:, :10] = True
    tokens, props = complete_and_validate(inv, fwd, cond, draft, keep, DEV, cond_scale=1.0, timesteps=5, forward_timesteps=4,
                                          num_resamples=2, X_norm_factor=16.0, forward_noise=NoiseSource(seed=4), seed=3)
    assert tokens.shape == (4, 32) and tokens.dtype == torch.int64 and props.shape == (4, 12) and props.device.type == "cuda"
    assert torch.isfinite(props).all() and torch.equal(tokens.cpu()[keep], draft[keep])
    # the same through the two public calls
    again = inv.inpaint_tokens(cond, DEV, draft, keep, cond_scale=1.0, timesteps=5, num_resamples=2, seed=3)
    assert torch.equal(again, tokens)
    assert torch.equal(predict_properties_from_tokens(fwd, tokens, DEV, timesteps=4, X_norm_factor=16.0, noise=NoiseSource(seed=4)),
                       props)
