"""CPU: the host side of a guidance scale per sample -- the normaliser (guidance_rows), the unchanged class surface, the pass-through
of the validation chains, the new C ABI entry and its no-device argument checks, the shape inference of mdt::cfg_mix_rows, the
fixture recorded from the real reference against the oracle, guidance_sweep's row order, and the per-step seam's refusal."""
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
from helpers import noise_fns, oracle_cfg, synth_sd, to_t
import moleculediffusiontransformer_amd as M
from moleculediffusiontransformer_amd import runtime as rt
from moleculediffusiontransformer_amd.diffusion import guidance_rows, is_guided
from oracle import unet_oracle as O

ORACLE_TOL = 2e-6    # the oracle's bound against the reference (test_oracle_golden.py)


# ----------------------------------------------------------------------------------------------------------------------
# the normaliser
# ----------------------------------------------------------------------------------------------------------------------
def test_a_number_or_a_0_dim_value_is_the_scalar_path():
    for v, want in ((7.5, 7.5), (2, 2.0), (0, 0.0), (-1.5, -1.5), (np.float32(2.5), 2.5), (np.float64(0.1), 0.1), (np.int64(3), 3.0),
                    (torch.tensor(7.5), 7.5), (torch.tensor(2), 2.0), (np.array(1.25), 1.25),
                    (torch.tensor(0.1, dtype=torch.float64), 0.1)):
        got = guidance_rows(v, 4)
        assert type(got) is float and got == want, v
    assert not is_guided(guidance_rows(1, 4)) and is_guided(guidance_rows(1.5, 4)) and is_guided(guidance_rows(0, 4))


def test_one_value_per_sample_is_an_fp32_cpu_tensor():
    want = torch.tensor([1.0, 2.0, 0.5, 7.5], dtype=torch.float32)
    forms = ([1, 2, 0.5, 7.5], (1.0, 2.0, 0.5, 7.5), np.array([1, 2, 0.5, 7.5]), np.array([1, 2, 0.5, 7.5], dtype=np.float32),
             torch.tensor([1, 2, 0.5, 7.5]), torch.tensor([1, 2, 0.5, 7.5], dtype=torch.float64),
             torch.tensor([1, 2, 0.5, 7.5], dtype=torch.float16), [torch.tensor(1.0), 2, np.float32(0.5), 7.5])
    for v in forms:
        got = guidance_rows(v, 4)
        assert isinstance(got, torch.Tensor) and got.dtype == torch.float32 and got.device.type == "cpu", type(v)
        assert got.shape == (4,) and got.is_contiguous() and torch.equal(got, want)
        assert is_guided(got)
    ints = guidance_rows([1, 2, 3], 3)
    assert ints.dtype == torch.float32 and ints.tolist() == [1.0, 2.0, 3.0]
    src = torch.tensor([1.0, 2.0])
    got = guidance_rows(src, 2)
    got[0] = 5.0
    assert src[0] == 1.0                              # the caller's tensor is not aliased
    assert guidance_rows(guidance_rows([1, 2, 3], 3), 3).tolist() == [1.0, 2.0, 3.0]      # idempotent
    assert guidance_rows([0.1, 0.2], 2).tolist() == [float(np.float32(0.1)), float(np.float32(0.2))]


def test_all_equal_values_collapse_to_the_float():
    for v, want in (([2.0, 2.0, 2.0], 2.0), (torch.ones(3), 1.0), (np.full(3, 7.5), 7.5), ([0.1] * 3, float(np.float32(0.1))),
                    ([0.0, -0.0, 0.0], 0.0)):
        got = guidance_rows(v, 3)
        assert type(got) is float and got == want
    assert guidance_rows([4.0], 1) == 4.0 and type(guidance_rows([4.0], 1)) is float
    assert not is_guided(guidance_rows(torch.ones(5), 5))
    assert guidance_rows([], 0) == 1.0 and guidance_rows(torch.empty(0), 0) == 1.0        # an empty batch: nothing to guide


@pytest.mark.parametrize("bad,what", [
    ([1.0, 2.0], "got 2 values"), ([1.0, 2.0, 3.0, 4.0], "got 4 values"), ([], "got 0 values"),
    ([[1.0, 2.0, 3.0]], "dimensions"), (torch.ones(3, 1), "dimensions"), (np.ones((1, 3)), "dimensions"),
    ([1.0, float("nan"), 2.0], "NaN"), ([1.0, float("inf"), 2.0], "NaN or an infinity"), (float("nan"), "nan"),
    (float("-inf"), "inf"), (torch.tensor(float("nan")), "nan"), (torch.tensor([1e39, 1.0, 2.0], dtype=torch.float64), "infinity"),
    (True, "bool"), ([True, False, True], "bool"), (torch.tensor(True), "bool"), (np.array([True, False, True]), "bool"),
    (1j, "complex"), (torch.tensor([1j, 2, 3]), "complex"), (np.array([1j, 2, 3]), "complex"),
    ("7.5", "str"), (None, "NoneType"), ({"a": 1}, "dict")])
def test_everything_else_is_refused_by_name(bad, what):
    with pytest.raises(ValueError, match=what) as e:
        guidance_rows(bad, 3)
    assert str(e.value).startswith("cond_scale must")
    with pytest.raises(ValueError, match="^embedding_scale must"):
        guidance_rows(bad, 3, "embedding_scale")


# ----------------------------------------------------------------------------------------------------------------------
# the class surface
# ----------------------------------------------------------------------------------------------------------------------
def test_signatures_and_defaults_are_unchanged():
    sig = lambda f: [(n, p.default, p.kind) for n, p in inspect.signature(f).parameters.items()]    # noqa: E731
    P, K, E = inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.KEYWORD_ONLY, inspect.Parameter.empty
    tail = [("noise", None, K), ("trace", None, K), ("timer", None, K), ("sampler", None, K), ("sigma_schedule", None, K)]
    head = [("self", E, P), ("sequences", E, P), ("device", E, P)]
    for cls, scale in ((M.QMDiffusion, 7.5), (M.QMDiffusionForward, 1.0), (M.AnalogDiffusionSparse, 7.5), (M.AnalogDiffusionFull, 7.5)):
        assert sig(cls.sample) == head + [("cond_scale", scale, P), ("timesteps", 100, P), ("clamp", False, P)] + tail, cls
        assert sig(cls.sample_tokens) == head + [("cond_scale", None, P), ("timesteps", 100, P), ("clamp", False, P), ("noise", None, K),
                                                 ("return_sample", False, K), ("sampler", None, K), ("sigma_schedule", None, K)]
        assert sig(cls.inpaint) == head + [("cond_scale", 7.5, P), ("timesteps", 100, P), ("num_resamples", 1, P), ("inpaint", None, P),
                                           ("in_paint_mask", None, P), ("draw", None, K), ("seed", None, K), ("sample0", 0, K)]
        assert sig(cls.inpaint_tokens) == head + [("draft_tokens", E, P), ("keep_mask", E, P), ("cond_scale", 7.5, P), ("timesteps", 100, P),
                                                  ("num_resamples", 1, P), ("draw", None, K), ("seed", None, K), ("sample0", 0, K),
                                                  ("return_sample", False, K)]
    assert [n for n, _, _ in sig(M.XDiffusion_x.sample)] == ["self", "noise", "num_steps", "sigma_schedule", "sampler", "clamp", "kwargs"]
    assert [n for n, _, _ in sig(M.XDiffusion_x.inpaint)] == ["self", "sigma_schedule", "sampler", "inpaint", "in_paint_mask", "num_steps",
                                                             "num_resamples", "kwargs"]
    gv, cv = inspect.signature(M.generate_and_validate).parameters, inspect.signature(M.complete_and_validate).parameters
    assert gv["cond_scale"].default == cv["cond_scale"].default == 1.0
    sw = inspect.signature(M.guidance_sweep).parameters
    assert list(sw) == ["model", "sequences", "cond_scales", "device", "tokens", "sample_kwargs"]
    assert sw["tokens"].kind is K and sw["tokens"].default is False and sw["sample_kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    # the whole-loop ops keep their schemas: the guidance scale stays a float there
    from moleculediffusiontransformer_amd import ops  # noqa: F401  (registers torch.ops.mdt.*)
    for name in ("sample", "sample_with", "inpaint_tokens", "unet_eval", "unet_eval_rows"):
        assert "float embedding_scale" in str(getattr(torch.ops.mdt, name).default._schema), name


def test_the_validation_chains_hand_cond_scale_on_as_given(monkeypatch):
    from moleculediffusiontransformer_amd import generative as G
    seen = {}

    class Inv:
        def inpaint_tokens(self, *a, **k):
            seen["inpaint"] = k
            return torch.full((2, 32), 3)

        def sample_tokens(self, *a, **k):
            seen["sample"] = k
            return torch.full((2, 32), 3)
    monkeypatch.setattr(G, "predict_properties_from_tokens", lambda mf, tok, dev, **k: seen.update(fwd=k) or "props")
    cond, draft, keep = torch.zeros(2, 12), torch.ones(2, 32, dtype=torch.long), torch.zeros(2, 32, dtype=torch.bool)
    for scales in ([1.0, 7.5], torch.tensor([2.0, 3.0]), np.array([1.0, 2.0]), 2.5):
        M.complete_and_validate(Inv(), "fwd", cond, draft, keep, "cpu", cond_scale=scales, timesteps=4)
        assert seen["inpaint"]["cond_scale"] is scales and seen["fwd"]["cond_scale"] == 1.0
        M.generate_and_validate(Inv(), "fwd", cond, "cpu", cond_scale=scales, timesteps=4)
        assert seen["sample"]["cond_scale"] is scales and seen["fwd"]["cond_scale"] == 1.0


def test_a_wrong_scale_is_refused_before_anything_runs():
    """No device is touched: the calls name a GPU this machine may not have, and the ValueError comes first."""
    m = M.QMDiffusion(max_length=32, pred_dim=16, channels=16, context_embedding_max_length=12, text_embed_dim=64,
                      embed_dim_position=64)
    seq = torch.zeros(3, 12)
    draft, keep = torch.zeros(3, 32, dtype=torch.long), torch.zeros(3, 32, dtype=torch.bool)
    for bad, what in (([1.0, 2.0], "got 2 values"), ([[1.0, 2.0, 3.0]], "dimensions"), ([1.0, float("nan"), 2.0], "NaN"),
                      ([True, False, True], "bool")):
        with pytest.raises(ValueError, match=what):
            m.sample(seq, "cuda:0", cond_scale=bad, timesteps=4)
        with pytest.raises(ValueError, match=what):
            m.sample_tokens(seq, "cuda:0", cond_scale=bad, timesteps=4)
        with pytest.raises(ValueError, match=what):
            m.inpaint(seq, "cuda:0", cond_scale=bad, timesteps=4, inpaint=torch.zeros(3, 16, 32),
                      in_paint_mask=torch.zeros(3, 16, 32, dtype=torch.bool), seed=1)
        with pytest.raises(ValueError, match=what):
            m.inpaint_tokens(seq, "cuda:0", draft, keep, cond_scale=bad, timesteps=4, seed=1)
        with pytest.raises(ValueError, match="^embedding_scale must"):
            m.diffusion.sample(None, 4, M.KarrasSchedule(0.001, 9.0, 3.0), M.ADPM2Sampler(rho=1), False,
                               embedding=torch.zeros(3, 12, 128), embedding_scale=bad)
        with pytest.raises(ValueError, match="^embedding_scale must"):
            m.diffusion.inpaint(M.KarrasSchedule(0.001, 9.0, 3.0), M.ADPM2Sampler(rho=1), torch.zeros(3, 16, 32),
                                torch.zeros(3, 16, 32, dtype=torch.bool), 4, 1, embedding=torch.zeros(3, 12, 128), embedding_scale=bad)
    # an empty batch with an empty scale list: empty results, nothing launched
    tok, x = m.inpaint_tokens(seq[:0], "cpu", draft[:0], keep[:0], cond_scale=[], return_sample=True)
    assert tok.shape == (0, 32) and x.shape == (0, 16, 32)


def test_the_per_step_seam_takes_one_scale():
    """A caller's fn, a sampler with its own step(), denoise_fn and net() called directly evaluate the network with ONE scale: a
    per-sample scale raises TypeError there, before any device work."""
    m = M.QMDiffusion(max_length=32, pred_dim=16, channels=16, context_embedding_max_length=12, text_embed_dim=64,
                      embed_dim_position=64)
    x, emb = torch.zeros(3, 16, 32), torch.zeros(3, 12, 128)
    scales = guidance_rows([1.0, 2.0, 7.5], 3)
    kd = m.diffusion.diffusion
    for s in (scales, [1.0, 2.0, 7.5], np.array([1.0, 2.0, 7.5])):
        with pytest.raises(TypeError, match="needs the fused loop"):
            kd.denoise_fn(x, sigma=torch.tensor(1.0), embedding=emb, embedding_scale=s)
        with pytest.raises(TypeError, match="needs the fused loop"):
            kd.denoise_fn(x, sigmas=torch.tensor([1.0, 2.0, 2.0]), embedding=emb, embedding_scale=s)
        with pytest.raises(TypeError, match="needs the fused loop"):
            kd.denoise_fn(x, sigmas=torch.tensor([1.0, 2.0, 2.0]), embedding=emb, embedding_scale=s, batched=True)
        with pytest.raises(TypeError, match="needs the fused loop"):
            m.unet(x, torch.tensor(0.3), embedding=emb, embedding_scale=s)
        with pytest.raises(TypeError, match="needs the fused loop"):
            m.unet(x, torch.tensor([0.3, 0.1, 0.2]), embedding=emb, embedding_scale=s, batched=True)

    class OwnStep(M.AEulerSampler):              # a subclass with its own step(): it gets the per-step path
        def step(self, x, fn, sigma, sigma_next, **kw):
            return fn(x, sigma=sigma)
    with pytest.raises(TypeError, match="needs the fused loop"):
        m.diffusion.sample(torch.zeros(3, 16, 32), 4, M.KarrasSchedule(0.001, 9.0, 3.0), OwnStep(), False, embedding=emb,
                           embedding_scale=[1.0, 2.0, 7.5])
    # a caller's fn around the model's denoiser
    ds = M.DiffusionSampler(kd, sampler=OwnStep(), sigma_schedule=M.KarrasSchedule(0.001, 9.0, 3.0), num_steps=4)
    with pytest.raises(TypeError, match="needs the fused loop"):
        ds(torch.zeros(3, 16, 32), embedding=emb, embedding_scale=scales)


# ----------------------------------------------------------------------------------------------------------------------
# the C ABI entry and the op
# ----------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_knows_mdt_cfg_mix_rows():
    hdr = open(os.path.join(ROOT, "include", "mdt_hip.h")).read()
    decl = re.search(r"\bint mdt_cfg_mix_rows\s*\(([^;]*)\);", hdr)
    assert decl is not None
    args = [a.strip() for a in decl.group(1).split(",")]
    assert len(args) == 7 == len(rt.SYMBOLS["mdt_cfg_mix_rows"][1])
    assert args[3] == "const float *scale" and args[4] == "int32_t B" and args[5] == "int64_t row_elems"
    assert re.search(r"#define MDT_ABI_VERSION 5\b", hdr) and rt.ABI_VERSION == 5       # an addition inside ABI version 5
    lib = rt.load_library()
    assert hasattr(lib, "mdt_cfg_mix_rows") and hasattr(lib, "mdt_cfg_mix") and lib.mdt_abi_version() == 5
    # argument checks that need no device
    assert lib.mdt_cfg_mix_rows(0, 0, 0, 0, 0, 64, 0) == 0                             # B <= 0: a no-op, whatever the rest
    assert lib.mdt_cfg_mix_rows(0, 0, 0, 0, -3, 30, 0) == 0
    for row_elems in (30, 0, -4, 2):
        assert lib.mdt_cfg_mix_rows(8, 8, 8, 8, 1, row_elems, 0) != 0
        assert b"mdt_cfg_mix_rows" in lib.mdt_last_error() and b"multiple of 4" in lib.mdt_last_error()
    for ptrs in ((0, 8, 8, 8), (8, 0, 8, 8), (8, 8, 0, 8), (8, 8, 8, 0)):
        assert lib.mdt_cfg_mix_rows(*ptrs, 1, 64, 0) != 0
        assert b"mdt_cfg_mix_rows: null pointer" in lib.mdt_last_error()


def test_cfg_mix_rows_op_shape_inference_and_refusals():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from moleculediffusiontransformer_amd import ops  # noqa: F401  (registers torch.ops.mdt.*)
    assert "mdt::cfg_mix_rows(Tensor cond, Tensor uncond, Tensor scale) -> Tensor" in str(torch.ops.mdt.cfg_mix_rows.default._schema)
    with FakeTensorMode():
        out = torch.ops.mdt.cfg_mix_rows(torch.empty(5, 32, 16), torch.empty(5, 32, 16), torch.empty(5))
        assert out.shape == (5, 32, 16) and out.dtype == torch.float32
        assert torch.ops.mdt.cfg_mix_rows(torch.empty(0, 32, 16), torch.empty(0, 32, 16), torch.empty(0)).shape == (0, 32, 16)
        assert torch.ops.mdt.cfg_mix_rows(torch.empty(3, 64, dtype=torch.float16), torch.empty(3, 64), torch.empty(3)).dtype == torch.float32
        with pytest.raises(RuntimeError, match="shape mismatch"):
            torch.ops.mdt.cfg_mix_rows(torch.empty(5, 32, 16), torch.empty(5, 32, 32), torch.empty(5))
        with pytest.raises(RuntimeError, match="scale holds 4 values"):
            torch.ops.mdt.cfg_mix_rows(torch.empty(5, 32, 16), torch.empty(5, 32, 16), torch.empty(4))
    # real tensors off the GPU: there is no CPU implementation
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        torch.ops.mdt.cfg_mix_rows(torch.zeros(5, 32, 16), torch.zeros(5, 32, 16), torch.ones(5))


# ----------------------------------------------------------------------------------------------------------------------
# the fixture against the oracle
# ----------------------------------------------------------------------------------------------------------------------
def fixture_cases():
    g = load_golden("guidance_rows.npz")
    for name, model, sampler, tag in zip(g["cases"], g["models"], g["samplers"], g["tags"]):
        name = str(name)
        yield name, str(model), str(sampler), str(tag), {k[len(name) + 1:]: v for k, v in g.items() if k.startswith(f"{name}_")}


def test_fixture_has_the_cases_of_the_generator():
    cases = {n: (m, s, g) for n, m, s, _, g in fixture_cases()}
    assert {n: v[:2] for n, v in cases.items()} == {"tiny_adpm2": ("tiny", "adpm2"), "tiny_aeuler": ("tiny", "aeuler"),
                                                    "cfg1_adpm2": ("cfg1", "adpm2")}
    assert cases["tiny_adpm2"][2]["scales"].tolist() == cases["tiny_aeuler"][2]["scales"].tolist() == [1.0, 2.0, 0.5, 7.5, 2.0]
    assert cases["cfg1_adpm2"][2]["scales"].tolist() == [7.5, 1.0, 2.0, 2.0, 1.0, 0.0, 3.0, 7.5]
    assert [int(cases[n][2]["timesteps"]) for n in ("tiny_adpm2", "tiny_aeuler", "cfg1_adpm2")] == [8, 8, 6]
    assert cases["tiny_adpm2"][2]["out"].shape == (5, 16, 32) and cases["cfg1_adpm2"][2]["out"].shape == (8, 16, 64)
    for _, _, g in cases.values():
        assert g["scales"].dtype == np.float32 and g["out"].dtype == np.float32 and int(g["ndraws"]) == int(g["timesteps"])
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "guidance_rows.npz")) < 100 * 1024


def oracle_aeuler(sd, cfg, noise, emb, T, step_noise, scale):
    """AEulerSampler.forward / step (diffusion.py:465-483) over the oracle's denoiser, as oracle.unet_oracle.adpm2_sample is
    ADPM2Sampler's."""
    with torch.no_grad():
        sigmas = O.karras_sigmas(T, dtype=noise.dtype)
        x = sigmas[0] * noise
        for i in range(T - 1):
            sigma, sigma_next = sigmas[i], sigmas[i + 1]
            sigma_up = math.sqrt(sigma_next ** 2 * (sigma ** 2 - sigma_next ** 2) / sigma ** 2)
            sigma_down = math.sqrt(sigma_next ** 2 - sigma_up ** 2)
            d = (x - O.denoise(sd, cfg, x, sigma, emb, scale)) / sigma
            x = x + d * (sigma_down - sigma)
            x = x + step_noise(i, x) * sigma_up
        return x


@pytest.mark.parametrize("name,model,sampler,tag,g", list(fixture_cases()), ids=lambda v: v if isinstance(v, str) else "")
def test_oracle_reproduces_the_fixture(name, model, sampler, tag, g):
    """Per distinct scale ONE oracle run of the whole batch on the recorded noise; row b of the run at scales[b], stitched, is the
    record at the oracle's bound.  The recorded rows of two different scales differ by far more than that."""
    sd, cfg = synth_sd(model), oracle_cfg(model)
    out_ref, scales, T = to_t(g["out"]), [float(s) for s in g["scales"]], int(g["timesteps"])
    init, step = noise_fns(tag, tuple(out_ref.shape))
    with torch.no_grad():
        emb = O.cond_embed(sd, cfg, to_t(g["seq"]))
    runs = {}
    for s in sorted(set(scales)):
        if sampler == "adpm2":
            runs[s] = O.adpm2_sample(sd, cfg, init, emb, T, step, s)
        else:
            runs[s] = oracle_aeuler(sd, cfg, init, emb, T, step, s)
    out = torch.stack([runs[s][b] for b, s in enumerate(scales)])
    err = float((out - out_ref).abs().max())
    print(f"\nguidance_rows {name}: max|oracle - reference| = {err:.3e} over {len(runs)} runs")
    assert err <= ORACLE_TOL
    for b, s in enumerate(scales):                   # a row taken from the run of another scale is not the record
        for other, o in runs.items():
            if other != s:
                assert float((o[b] - out_ref[b]).abs().max()) > 1e3 * ORACLE_TOL, (b, s, other)


# ----------------------------------------------------------------------------------------------------------------------
# guidance_sweep against a stand-in model
# ----------------------------------------------------------------------------------------------------------------------
class StandIn:
    """sample(): element [r, c, l] = 1000 * (first conditioning value of row r) + cond_scale[r] + c / 8 + l / 64."""

    def __init__(self):
        self.calls = []

    def sample(self, sequences, device, cond_scale=None, **kw):
        self.calls.append(("sample", sequences.clone(), device, cond_scale, kw))
        grid = torch.arange(2).view(1, 2, 1) / 8 + torch.arange(4).view(1, 1, 4) / 64
        return 1000 * sequences[:, :1, None] + torch.as_tensor(cond_scale).view(-1, 1, 1) + grid

    def sample_tokens(self, sequences, device, cond_scale=None, return_sample=False, **kw):
        self.calls.append(("sample_tokens", sequences.clone(), device, cond_scale, kw))
        tok = (10 * sequences[:, :1] + torch.as_tensor(cond_scale).view(-1, 1)).long().expand(-1, 4).contiguous()
        return (tok, self.sample(sequences, device, cond_scale)) if return_sample else tok


def test_guidance_sweep_row_order_and_reshape():
    seq = torch.tensor([[1.0, 9.0], [2.0, 9.0], [3.0, 9.0]])                       # B = 3 conditionings
    scales = [7.5, 1.0, 2.0, 7.5]                                                  # S = 4
    m = StandIn()
    out = M.guidance_sweep(m, seq, scales, "dev", timesteps=9, noise="ns")
    assert len(m.calls) == 1 and m.calls[0][0] == "sample" and m.calls[0][2] == "dev"
    _, seqs, _, cs, kw = m.calls[0]
    assert kw == dict(timesteps=9, noise="ns")
    assert torch.equal(seqs, seq.repeat(4, 1))                                     # row s * B + b is conditioning b ...
    assert isinstance(cs, torch.Tensor) and cs.dtype == torch.float32
    assert cs.tolist() == [7.5] * 3 + [1.0] * 3 + [2.0] * 3 + [7.5] * 3            # ... at cond_scales[s]
    assert out.shape == (4, 3, 2, 4)
    for s, scale in enumerate(scales):
        for b in range(3):
            assert float(out[s, b, 0, 0]) == 1000 * (b + 1) + scale
    assert torch.equal(out[0], out[3]) and out.is_contiguous()
    # tokens: one sample_tokens call; a tuple result is reshaped part by part
    m = StandIn()
    tok = M.guidance_sweep(m, seq, np.array(scales), "dev", tokens=True)
    assert [c[0] for c in m.calls] == ["sample_tokens"] and tok.shape == (4, 3, 4) and tok.dtype == torch.int64
    assert tok[:, :, 0].tolist() == [[17, 27, 37], [11, 21, 31], [12, 22, 32], [17, 27, 37]]
    tok2, x = M.guidance_sweep(StandIn(), seq, torch.tensor(scales), "dev", tokens=True, return_sample=True)
    assert torch.equal(tok2, tok) and torch.equal(x, out)
    # a sweep of equal scales still makes one call of S * B rows; one scale; none
    same = M.guidance_sweep(StandIn(), seq, [2.0, 2.0], "dev")
    assert same.shape == (2, 3, 2, 4) and torch.equal(same[0], same[1]) and float(same[0, 0, 0, 0]) == 1002.0
    assert M.guidance_sweep(StandIn(), seq, [3.0], "dev").shape == (1, 3, 2, 4)
    assert M.guidance_sweep(StandIn(), seq, [], "dev").shape == (0, 3, 2, 4)
    for bad in (2.0, [[1.0, 2.0]], torch.ones(2, 2)):
        with pytest.raises(ValueError, match="1-D"):
            M.guidance_sweep(StandIn(), seq, bad, "dev")
    for bad, what in (([1.0, float("nan")], "NaN"), ([True, False], "bool")):
        with pytest.raises(ValueError, match=what) as e:
            M.guidance_sweep(StandIn(), seq, bad, "dev")
        assert str(e.value).startswith("cond_scales must")
