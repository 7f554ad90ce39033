"""Drop-in class surface: QMDiffusion (generative.py:718-914) and QMDiffusionForward (:31-225).

Same constructor keywords, attributes (.unet, .diffusion, .fc1, .GELUact, .p_enc_1d, .max_length,
.pred_dim, ...), state_dict key layout (the U-Net appears under unet.*, diffusion.net.* and
diffusion.diffusion.net.*, as in the reference) and sample()/inpaint() signatures.  The sampling
path runs on an MI355X through libmdt_hip.so; there is no CPU implementation behind these classes.
"""
from __future__ import annotations

import os
from typing import Callable, NamedTuple, Optional

import torch
import torch.nn as nn

from . import ops, runtime as rt
from .compiler import compile_unet
from .diffusion import (FUSED_SAMPLERS, ADPM2Sampler, DiffusionInpainter, DiffusionSampler, KarrasSchedule, LogNormalDistribution,
                        NoiseSource, guidance_rows, is_guided, refine_start, require_fused_kind, run_adpm2_inpaint, run_refine,
                        run_sampler, scalar_guidance, scale_weights, scale_weights_rows, start_rows)
from .engine import UNetEngine, _require_gpu
from .modules import PositionalEncoding1D, UNetCFG1d
from .netspec import forward_unet_config, inverse_unet_config

Tensor = torch.Tensor


class KDiffusion_mod(nn.Module):
    """diffusion.py:770-844: Karras preconditioning around the net (alias 'k')."""

    alias = "k"

    def __init__(self, net: nn.Module, *, sigma_distribution, sigma_data: float, dynamic_threshold: float = 0.0):
        super().__init__()
        if not 0.0 <= dynamic_threshold <= 1.0:
            raise ValueError("dynamic_threshold is a quantile: 0 (static clamp to [-1, 1]) ... 1")
        self.net = net
        self.sigma_data = sigma_data
        self.sigma_distribution = sigma_distribution
        self.dynamic_threshold = dynamic_threshold
        self._owner = None

    def denoise_fn(self, x_noisy: Tensor, sigmas: Optional[Tensor] = None, sigma=None, *, embedding: Tensor,
                   embedding_scale: float = 1.0, batched: bool = False) -> Tensor:
        """diffusion.py:798-814: a scalar ``sigma`` (the sampling case) or one sigma per sample (``sigmas``, the
        training-time form; samples sharing a sigma are evaluated together).  ``batched=True`` (with ``sigmas``): ONE evaluation
        of the per-row program for the whole batch, whatever the number of distinct values -- equal to the default to rounding
        (1e-6 class: the ResNet blocks run through other kernels), not bit for bit."""
        if sigma is None and sigmas is None:
            raise AssertionError("Either sigma or sigmas must be provided")       # to_batch, diffusion.py:97
        if sigma is not None:
            return self._owner._denoise(x_noisy, sigma, embedding, embedding_scale)
        sig = torch.as_tensor(sigmas, dtype=torch.float32).flatten().cpu()
        if sig.numel() != x_noisy.shape[0]:
            raise AssertionError("sigmas must hold one value per sample")
        if batched:
            return self._owner._denoise_rows(x_noisy, sig, embedding, embedding_scale)
        out = torch.empty_like(x_noisy, dtype=torch.float32)
        for v in torch.unique(sig):
            rows = (sig == v).nonzero().flatten().to(x_noisy.device)
            out[rows] = self._owner._denoise(x_noisy[rows], v, embedding[rows], embedding_scale)
        return out

    def forward(self, x: Tensor, noise: Optional[Tensor] = None, *, embedding: Tensor, **kwargs) -> Tensor:
        """Training loss of KDiffusion_mod.forward (diffusion.py:820-844) -- plain PyTorch with autograd (train.py);
        the MI355X kernels serve sampling only."""
        from .train import kdiffusion_loss
        return kdiffusion_loss(self._owner, x, noise, embedding, **kwargs)


class XDiffusion_x(nn.Module):
    """diffusion.py:706-767: picks the diffusion class by alias ('k' -> KDiffusion_mod) and exposes
    sample()/inpaint() with sampler and schedule objects."""

    def __init__(self, type: str, net: nn.Module, **kwargs):
        super().__init__()
        if type != "k":
            raise NotImplementedError(f"type='{type}': only the 'k' diffusion used by QMDiffusion* is built")
        self.net = net
        self.diffusion = KDiffusion_mod(net=net, **kwargs)

    def forward(self, *args, **kwargs):
        return self.diffusion(*args, **kwargs)

    def sample(self, noise, num_steps: int, sigma_schedule, sampler, clamp: bool, **kwargs) -> Tensor:
        """diffusion.py:724-741: builds a DiffusionSampler and calls it.  ``noise``: the initial draw (B, C, L) as in the
        reference, a NoiseSource, or None (drawn like generative.py:853).  ``embedding_scale``: one guidance scale, or one per
        sample (guidance_rows; the fused loops only)."""
        _normalise_scale(kwargs)
        diffusion_sampler = DiffusionSampler(diffusion=self.diffusion, sampler=sampler, sigma_schedule=sigma_schedule,
                                             num_steps=num_steps, clamp=clamp)
        return diffusion_sampler(noise, **kwargs)

    def inpaint(self, sigma_schedule, sampler, inpaint, in_paint_mask, num_steps: int, num_resamples: int,
                **kwargs) -> Tensor:
        """diffusion.py:744-767: builds a DiffusionInpainter and calls it.  ``embedding_scale`` as sample()."""
        _normalise_scale(kwargs)
        inpainter = DiffusionInpainter(diffusion=self.diffusion, sampler=sampler, sigma_schedule=sigma_schedule,
                                       num_steps=num_steps, num_resamples=num_resamples)
        return inpainter(inpaint, in_paint_mask, **kwargs)


def _normalise_scale(kwargs: dict) -> None:
    """embedding_scale of a sample() / inpaint() call in guidance_rows' form, checked against the embedding's batch."""
    emb = kwargs.get("embedding")
    if "embedding_scale" in kwargs and isinstance(emb, torch.Tensor):
        kwargs["embedding_scale"] = guidance_rows(kwargs["embedding_scale"], emb.shape[0], "embedding_scale")


class _FusedLoop:
    """What ADPM2Sampler.forward / inpaint and AEulerSampler / KarrasSampler.forward call when the denoiser belongs to a
    QMDiffusion* model: the whole loop on the fused path (run_sampler / run_adpm2_inpaint) instead of one callback per
    evaluation."""

    def __init__(self, owner, kwargs: dict, extra: dict):
        unknown = set(kwargs) - {"embedding", "embedding_scale"}
        if unknown or "embedding" not in kwargs:
            raise TypeError(f"denoise_fn takes embedding= and embedding_scale= (got {sorted(kwargs)})")
        self.owner, self.kw, self.extra = owner, kwargs, extra

    def sample(self, noise, sampler, sigmas, num_steps):
        o, emb = self.owner, self.kw["embedding"]
        if emb.shape[0] == 0:                       # nothing to generate (the reference returns an empty tensor too)
            return torch.empty(0, o.pred_dim, o.max_length, device=emb.device)
        scale = guidance_rows(self.kw.get("embedding_scale", 1.0), emb.shape[0], "embedding_scale")
        eng = o.engine(emb.device, emb.shape[1], emb.shape[0] * (2 if is_guided(scale) else 1))
        ns = o._noise_source(noise, emb.shape[0], emb.device)
        x, kd = self.extra, o.diffusion.diffusion
        clamp, tok = bool(x.get("clamp", False)), x.get("tokens")
        plain = ns.steps is None and x.get("trace") is None and x.get("timer") is None and not isinstance(scale, torch.Tensor)
        if not (plain and any(type(sampler) is k.cls for k in FUSED_SAMPLERS.values())):
            return run_sampler(eng, emb, o.pred_dim, num_steps, ns, sigmas, sampler, kd.sigma_data, scale, clamp, x.get("trace"),
                               x.get("timer"), tok, float(kd.dynamic_threshold))
        # the plain call (counter-based step noise, nothing to record, one guidance scale) with a sampler of exactly one of the
        # three classes: the whole loop as ONE custom op, mdt::sample for ADPM2 (it stays ADPM2's), mdt::sample_with for the other two
        init = None if ns.init is None else ns.init.to(device=emb.device, dtype=torch.float32)
        head = (emb, init, None, torch.as_tensor(sigmas, dtype=torch.float32).cpu(), ops.register_engine(eng), o.pred_dim)
        rest = (float(kd.sigma_data), float(scale), clamp, int(ns.seed or 0), int(ns.sample0), tok is not None,
                float(kd.dynamic_threshold))
        if type(sampler) is ADPM2Sampler:
            out, t = torch.ops.mdt.sample(*head, float(sampler.rho), *rest)
        else:
            out, t = torch.ops.mdt.sample_with(*head, *ops.sampler_spec(sampler), *rest)
        if tok is not None:
            tok.copy_(t)
        return out

    def inpaint(self, source, mask, sampler, sigmas, num_steps, num_resamples):
        o, emb = self.owner, self.kw["embedding"]
        scale = guidance_rows(self.kw.get("embedding_scale", 1.0), emb.shape[0], "embedding_scale")
        eng = o.engine(emb.device, emb.shape[1], emb.shape[0] * (2 if is_guided(scale) else 1))
        draw, seed = self.extra.get("draw"), self.extra.get("seed")
        if draw is None and seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        sample0, tok, kd = int(self.extra.get("sample0") or 0), self.extra.get("tokens"), o.diffusion.diffusion
        if source.is_floating_point():
            return run_adpm2_inpaint(eng, emb, source, mask, num_steps, num_resamples, draw, seed, sigmas, sampler, kd.sigma_data,
                                     scale, sample0, float(kd.dynamic_threshold), tokens=tok)
        # a draft of token ids (inpaint_tokens): without a draw callback and with one guidance scale the whole loop is ONE custom
        # op, as mdt::sample is
        if draw is None and type(sampler) is ADPM2Sampler and not isinstance(scale, torch.Tensor):
            x, t = torch.ops.mdt.inpaint_tokens(emb, source, mask, torch.as_tensor(sigmas, dtype=torch.float32).cpu(),
                                                ops.register_engine(eng), o.pred_dim, int(num_resamples), float(sampler.rho),
                                                float(kd.sigma_data), float(scale), int(seed), sample0,
                                                float(kd.dynamic_threshold))
            if tok is not None:
                tok.copy_(t)
            return x
        return run_adpm2_inpaint(eng, emb, None, None, num_steps, num_resamples, draw, seed, sigmas, sampler, kd.sigma_data, scale,
                                 sample0, float(kd.dynamic_threshold), draft=source, keep=mask, pred_dim=o.pred_dim, tokens=tok)


class _QMBase(nn.Module):
    _inverse = True

    def _init_common(self, max_length, channels, pred_dim, unet, context_embedding_max_length, unet_type,
                     pos_emb_fourier, pos_emb_fourier_add, text_embed_dim, embed_dim_position):
        self.unet_type = unet_type
        self.fc1 = nn.Linear(1, text_embed_dim)
        self.GELUact = nn.GELU()
        self.pos_emb_fourier = pos_emb_fourier
        self.pos_emb_fourier_add = pos_emb_fourier_add
        self._text_dim = text_embed_dim
        self._pos_dim = 0
        self._pos_add = bool(pos_emb_fourier and pos_emb_fourier_add)
        if pos_emb_fourier:
            if pos_emb_fourier_add:
                # x + p_enc_1d(x): the encoding returns its first text_embed_dim columns (transformer.py:3470), so any
                # text_embed_dim <= embed_dim_position works as in the reference; a larger one does not broadcast there either
                if text_embed_dim > embed_dim_position:
                    raise RuntimeError("pos_emb_fourier_add=True needs text_embed_dim <= embed_dim_position "
                                       "(x + p_enc_1d(x) does not broadcast otherwise, generative.py:846)")
            else:
                text_embed_dim = text_embed_dim + embed_dim_position
            self._pos_dim = embed_dim_position
            self.p_enc_1d = PositionalEncoding1D(embed_dim_position)
        self.max_length = max_length
        self.pred_dim = pred_dim
        if unet_type != "cfg":
            raise NotImplementedError("only unet_type='cfg' (UNetCFG1d) is on the MI355X sampling path")
        if unet is not None:
            if not isinstance(unet, UNetCFG1d):
                raise TypeError("unet must be a moleculediffusiontransformer_amd UNetCFG1d")
            self.unet = unet
        else:
            self.unet = UNetCFG1d(self._unet_config(pred_dim, channels, text_embed_dim, context_embedding_max_length))
        self.diffusion = XDiffusion_x(type="k", net=self.unet,
                                      sigma_distribution=LogNormalDistribution(mean=-1.2, std=1.2),
                                      sigma_data=0.1, dynamic_threshold=0.0)
        object.__setattr__(self.diffusion.diffusion, "_owner", self)
        self.unet._evaluator = self._unet_call
        # 'bf16x3': split-bf16 MFMA GEMMs (fp32-class accuracy, ~5x the fp32-MFMA rate); 'f32': exact fp32 MFMA
        self.gemm_mode = os.environ.get("MDT_GEMM", "bf16x3")
        # form of the 256-channel transformers: 'auto' (by the batch of each call), 'wide', 'narrow' (see _wide)
        self.kernel_choice = {"1": "wide", "0": "narrow"}.get(os.environ.get("MDT_TF256", "auto"), "auto")
        # A pair hand-off that times out (a partner workgroup was not resident: compute units held by another stream / process)
        # leaves garbage rows and a status word on the device.  By default every sampling call and every net() / denoise_fn()
        # evaluation waits for that word before it returns (one event wait per call) and raises RuntimeError.  A pipelined caller
        # that issues calls back to back may set this True (or MDT_DEFER_HANDOFF=1): the word is then looked at by the NEXT call,
        # or by engine.handoff_check(wait=True) when the caller synchronises anyway.
        self.defer_handoff_check = os.environ.get("MDT_DEFER_HANDOFF", "0") == "1"
        self._engine: Optional[UNetEngine] = None
        self._engines = {}               # wide (bool) -> UNetEngine, for the current parameter values
        self._engine_key = None
        self.sampler_stats = {}

    def _unet_config(self, pred_dim, channels, ctx_features, ctx_max_length):
        mk = inverse_unet_config if self._inverse else forward_unet_config
        return mk(pred_dim, channels, ctx_features, ctx_max_length)

    # ------------------------------------------------------------------ engine management
    def _param_key(self, device, n_ctx):
        # every call asks whether the compiled engine still belongs to the parameter VALUES (an optimiser step or load_state_dict
        # bumps _version, .to() moves the storage).  The Parameter objects themselves are fixed once the module is built, so the
        # walk over the module tree (766 parameters in ~400 modules: milliseconds, visible to net() / denoise_fn seam users at
        # small batches) happens once; per call only data_ptr / _version of the cached list are read.
        cached = self.__dict__.get("_plist")
        if cached is None or cached[0] is not self.unet:                 # (a caller may assign another U-Net module)
            cached = self.__dict__["_plist"] = (self.unet, list(self.unet.parameters()))
        ps = cached[1]
        return (str(device), n_ctx, self.gemm_mode, tuple((p.data_ptr(), p._version) for p in ps))

    def _wide(self, batch: Optional[int]) -> bool:
        """Which form of the 256-channel transformers to run (compiler.py: MDT_TF256).  With the heads split over workgroup PAIRS
        (k_tf256 NSPLIT = 2) a batch of up to 4096 rows at that level (1024 samples of 4 tokens) fills the chip;
        above, the whole-transformer launch without the split (measured against the split forms: +10 % at 2048, +7 % at 4096
        samples).  The two forms add the heads' partial sums in different orders, so they agree to
        rounding (1e-6 class), not bit for bit: ``kernel_choice`` = 'wide' / 'narrow' pins one of them for every batch size
        (what a sharded run does, distributed.sample_sharded / pin_kernel_choice); 'auto' decides per call."""
        if self.kernel_choice in ("wide", "narrow"):
            return self.kernel_choice == "wide"
        cfg = self.unet.config
        t256 = None
        length = self.max_length // cfg.patch_size
        for lvl in range(cfg.num_layers + 1):
            if cfg.level_channels(lvl) == 256:
                t256 = length
            if lvl < cfg.num_layers:
                length //= cfg.factors[lvl]
        # pair-split launches need both workgroups of a pair running at the same time: 2 workgroups per 32 rows, and the device
        # keeps rt.pair_capacity() of them resident at once (compute units x occupancy, asked from the device: 256 on an MI355X,
        # i.e. 4096 rows).  The narrow form is used while ONE launch holds the level; above, the whole-transformer form is faster
        # (a pinned 'narrow' stays correct at any batch: launch_tf256 splits it into launches that fit, csrc/k_tf256.hip)
        if not batch or t256 is None:
            return False
        return 2 * ((batch * t256 + 31) // 32) > rt.pair_capacity()

    def pin_kernel_choice(self, batch: Optional[int]) -> str:
        """Resolve 'auto' for a batch of ``batch`` U-Net rows (samples, doubled under guidance) and keep that choice for every
        later call, whatever its batch: per-sample results then do not depend on how a batch is split over calls or ranks.
        ``batch`` None releases the pin.  Returns the choice now in force."""
        if batch is None:
            self.kernel_choice = "auto"
        else:
            self.kernel_choice = "auto"
            self.kernel_choice = "wide" if self._wide(batch) else "narrow"
        return self.kernel_choice

    def engine(self, device, n_ctx: Optional[int] = None, batch: Optional[int] = None, rows: bool = False) -> UNetEngine:
        """Compiled-program engine for the current parameter values on `device` (rebuilt after an optimiser step or
        load_state_dict), `n_ctx` conditioning tokens and the kernel choice that fits `batch` U-Net rows (see _wide).
        ``rows``: the engine of the per-row programs (one noise level per sample: batched=True, eval_loss), compiled on first
        use and kept next to the sampling engine -- a second copy of the packed weights that sampling-only users never pay."""
        device = torch.device(device)
        _require_gpu(device)
        n_ctx = self.unet.config.ctx_max_length if n_ctx is None else n_ctx
        if n_ctx > self.unet.config.ctx_max_length:
            raise AssertionError("Input sequence length must be <= max_length")   # FixedEmbedding, modules.py:1194
        wide = self._wide(batch)
        key = self._param_key(device, n_ctx)
        if self._engine_key != key:                  # parameters changed: every cached engine is stale
            self._engines = {}
            self._engine_key = key
        slot = (wide, "rows") if rows else wide
        if slot not in self._engines:
            sd = {k: v.detach().float().cpu() for k, v in self.unet.state_dict().items()}
            compiled = compile_unet(self.unet.config, self.max_length, n_ctx, sd, gemm_mode=self.gemm_mode, tf256=wide, rows=rows)
            self._engines[slot] = UNetEngine(compiled, device)
        eng = self._engines[slot]
        eng.sync_handoff_check = not self.defer_handoff_check
        if not rows:
            self._engine = eng
        return eng

    # ------------------------------------------------------------------ conditioning prelude
    def _embed(self, sequences: Tensor, device) -> Tensor:
        """generative.py:838-850 / :149-161 on the device (torch.ops.mdt.cond_embed -> mdt_cond_embed)."""
        device = torch.device(device)
        _require_gpu(device)
        seq = sequences.detach().float().to(device)
        inv = self.p_enc_1d.inv_freq.detach().float().to(device) if self._pos_dim else None
        return torch.ops.mdt.cond_embed(seq, self.fc1.weight.detach().to(device), self.fc1.bias.detach().to(device), inv,
                                        self._pos_dim, self._pos_add)

    # ------------------------------------------------------------------ seams used by the wrappers above
    def _noise_source(self, noise, B, device, sample0=0):
        if isinstance(noise, NoiseSource):
            return noise
        # default: initial noise from the CPU global generator exactly as generative.py:853 does; the
        # per-step draws come from the counter-based device generator seeded from the same CPU generator
        init = torch.randn(B, self.pred_dim, self.max_length) if noise is None else noise
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        ns = NoiseSource(seed=seed, sample0=sample0)
        ns.init = init
        return ns

    def _fused_adapter(self, kwargs: dict, extra: dict) -> _FusedLoop:
        return _FusedLoop(self, kwargs, extra)

    def _unet_call(self, x: Tensor, time, embedding: Tensor, embedding_scale: float = 1.0, batched: bool = False) -> Tensor:
        """net(x, time, embedding=..., embedding_scale=...) (modules.py:1228-1255); x is (B, C, L) as in the reference,
        ``time`` a scalar or one value per row (rows sharing a time value are evaluated together; ``batched=True``: all rows in
        ONE evaluation of the per-row program)."""
        embedding_scale = scalar_guidance(embedding_scale, "net()")
        t = torch.as_tensor(time, dtype=torch.float32).flatten().cpu()
        B = x.shape[0]
        if t.numel() not in (1, B):
            raise ValueError(f"time must be a scalar or hold one value per sample (got {t.numel()} for batch {B})")
        if batched:
            device = x.device
            _require_gpu(device)
            eng = self.engine(device, embedding.shape[1], B, rows=True)
            with torch.no_grad():
                xin = torch.ops.mdt.precond_in(x, 1.0, eng.c.in_pad)
                pred = torch.ops.mdt.unet_eval_rows(xin, embedding, t.expand(B).to(device), float(embedding_scale),
                                                    ops.register_engine(eng))
                return pred[:, :, :x.shape[1]].transpose(1, 2).contiguous()
        if t.numel() > 1 and not bool((t == t[0]).all()):
            out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
            for v in torch.unique(t):
                rows = (t == v).nonzero().flatten().to(x.device)
                out[rows] = self._unet_call(x[rows], v, embedding[rows], embedding_scale)
            return out
        device = x.device
        _require_gpu(device)
        eng = self.engine(device, embedding.shape[1], x.shape[0])
        C = x.shape[1]
        with torch.no_grad():
            xin = torch.ops.mdt.precond_in(x, 1.0, eng.c.in_pad)
            pred = torch.ops.mdt.unet_eval(xin, embedding, float(t[0]), float(embedding_scale), ops.register_engine(eng))
            return pred[:, :, :C].transpose(1, 2).contiguous()

    def _denoise(self, x_noisy: Tensor, sigma, embedding: Tensor, embedding_scale: float = 1.0) -> Tensor:
        """KDiffusion_mod.denoise_fn for a scalar sigma (diffusion.py:798-814) as three ops: input scaling, the network,
        output mix + clip."""
        embedding_scale = scalar_guidance(embedding_scale, "denoise_fn")
        device = x_noisy.device
        _require_gpu(device)
        eng = self.engine(device, embedding.shape[1], x_noisy.shape[0])
        w = scale_weights(torch.as_tensor(sigma, dtype=torch.float32).cpu(), self.diffusion.diffusion.sigma_data)
        with torch.no_grad():
            xin = torch.ops.mdt.precond_in(x_noisy, w.c_in, eng.c.in_pad)
            pred = torch.ops.mdt.unet_eval(xin, embedding, w.c_noise, float(embedding_scale), ops.register_engine(eng))
            return torch.ops.mdt.precond_out(x_noisy, pred, w.c_skip, w.c_out, float(self.diffusion.diffusion.dynamic_threshold))

    def _denoise_rows(self, x_noisy: Tensor, sigmas: Tensor, embedding: Tensor, embedding_scale: float = 1.0) -> Tensor:
        """KDiffusion_mod.denoise_fn with one sigma per sample (diffusion.py:798-814) as ONE per-row evaluation: the per-sample
        coefficients are computed on the host in the reference's fp32 expressions and uploaded once."""
        embedding_scale = scalar_guidance(embedding_scale, "denoise_fn")
        device = x_noisy.device
        _require_gpu(device)
        B = x_noisy.shape[0]
        eng = self.engine(device, embedding.shape[1], B, rows=True)
        w = scale_weights_rows(sigmas, self.diffusion.diffusion.sigma_data).packed().to(device)
        with torch.no_grad():
            xin = torch.ops.mdt.precond_in_rows(x_noisy, w[1], eng.c.in_pad)
            pred = torch.ops.mdt.unet_eval_rows(xin, embedding, w[4], float(embedding_scale), ops.register_engine(eng))
            return torch.ops.mdt.precond_out_rows(x_noisy, pred, w[2], w[3], float(self.diffusion.diffusion.dynamic_threshold))

    def _loss_target(self, output: Tensor) -> Tensor:
        """What forward() hands to the diffusion as the clean sample (the Analog* wrappers slice and pad `output`)."""
        return output

    def eval_loss(self, sequences, output, device, *, sigmas: Optional[Tensor] = None, noise: Optional[Tensor] = None,
                  seed: Optional[int] = None, per_sample: bool = False) -> Tensor:
        """The value of ``forward(sequences, output)`` -- conditioning prelude + KDiffusion_mod.forward (diffusion.py:820-844) at
        embedding_scale 1, honouring ``dynamic_threshold`` -- computed under no_grad on the MI355X kernels: noising, ONE per-row
        U-Net evaluation, fused clip + weighted MSE.  Returns a 0-dim tensor on ``device``, or with ``per_sample`` the (B,)
        weighted losses whose mean it is.

        ``sigmas`` (B,) / ``noise`` (B, C, L): given, or drawn from torch's global CPU generator in the reference's order (sigmas,
        diffusion.py:824, then noise, :828), so that under one torch.manual_seed the value is forward()'s of a CPU copy of the
        model.  ``seed`` (without ``noise``): the counter-based device generator keyed by (seed, sample index) instead.
        An empty batch raises ValueError (the reference's mean over no samples is nan).  There is no CPU fallback."""
        device = torch.device(device)
        _require_gpu(device)
        kd = self.diffusion.diffusion
        with torch.no_grad():
            x0 = self._loss_target(output.detach()).float()
            B = x0.shape[0]
            if B == 0:
                raise ValueError("eval_loss needs at least one sample")
            if tuple(x0.shape[1:]) != (self.pred_dim, self.max_length):
                raise ValueError(f"output is {tuple(x0.shape)}, the model diffuses (B, {self.pred_dim}, {self.max_length})")
            if sigmas is None:
                sigmas = kd.sigma_distribution(num_samples=B)
            if noise is None and seed is None:
                noise = torch.randn(x0.shape, dtype=torch.float32)
            w = scale_weights_rows(sigmas, kd.sigma_data)
            if w.sigmas.numel() != B:
                raise AssertionError("sigmas must hold one value per sample")
            emb = self._embed(sequences, device)
            eng = self.engine(device, emb.shape[1], B, rows=True)
            nz = None if noise is None else noise.detach().to(device=device, dtype=torch.float32)
            losses = torch.ops.mdt.eval_loss(x0.to(device), nz, emb, w.packed().to(device), ops.register_engine(eng),
                                             float(kd.dynamic_threshold), int(seed or 0), 0)
            return losses if per_sample else losses.mean()

    # ------------------------------------------------------------------ public API (reference signatures)
    def forward(self, sequences, output):
        """Training loss (generative.py:812-833 / :120-143): conditioning prelude + KDiffusion_mod.forward, plain PyTorch
        with autograd on whatever device the parameters live on (train.py).  Not on the MI355X sampling path."""
        from .train import conditioning_embedding
        x = conditioning_embedding(self, sequences)
        return self.diffusion(output, embedding=x)

    def _do_sample(self, sequences, device, cond_scale, timesteps, clamp, noise=None, trace=None, timer=None, tokens=None,
                   sampler=None, sigma_schedule=None):
        """``sampler`` / ``sigma_schedule`` None: the objects every sample() of the reference hard-codes (generative.py:855-858).
        ``cond_scale``: one guidance scale for the batch, or one per sample (a 1-D list / tuple / ndarray / tensor of B values,
        diffusion.guidance_rows): row b is then row b of the call at cond_scale[b] -- bit for bit when ``kernel_choice`` is pinned,
        to rounding under 'auto' (the per-sample call asks for the engine of 2 B rows, the call at scale 1 for B)."""
        cond_scale = guidance_rows(cond_scale, sequences.shape[0])          # (refused before anything is launched)
        emb = self._embed(sequences, device)
        if sampler is None:
            sampler = ADPM2Sampler(rho=1)
        if sigma_schedule is None:
            sigma_schedule = KarrasSchedule(sigma_min=0.001, sigma_max=9.0, rho=3.0)
        return self.diffusion.sample(num_steps=timesteps, sampler=sampler, sigma_schedule=sigma_schedule,
                                     clamp=clamp, noise=noise, embedding=emb, embedding_scale=cond_scale,
                                     trace=trace, timer=timer, tokens=tokens)

    def sample_tokens(self, sequences, device, cond_scale=None, timesteps=100, clamp=False, *, noise=None,
                      return_sample: bool = False, sampler=None, sigma_schedule=None):
        """sample() followed by the decode step of the reference's callers (sample_loop_generative / generate_from_conditioning,
        generative.py:1212-1213, :1690-1691: ``permute(0, 2, 1)`` then ``argmax(dim=2)``), with the argmax taken inside the
        last sampler update: returns (B, max_length) int64 token ids on ``device`` (and the fp32 sample if asked)."""
        if cond_scale is None:
            cond_scale = 7.5 if self._inverse else 1.0
        B = sequences.shape[0]
        cond_scale = guidance_rows(cond_scale, B)
        tok = torch.zeros(B, self.max_length, dtype=torch.int32, device=device)
        x = self._do_sample(sequences, device, cond_scale, timesteps, clamp, noise, tokens=tok if B else None,
                            sampler=sampler, sigma_schedule=sigma_schedule)
        tok = tok.long()
        return (tok, x) if return_sample else tok

    def inpaint(self, sequences, device, cond_scale=7.5, timesteps=100, num_resamples=1, inpaint=None,
                in_paint_mask=None, *, draw=None, seed=None, sample0=0):
        """``sample0``: the global index of this call's first sample (seed mode: the counter-based draws are keyed by
        sample0 + b, so a batch split over calls or ranks returns the rows of the whole batch).  ``cond_scale``: one guidance
        scale, or one per sample, as sample()."""
        cond_scale = guidance_rows(cond_scale, sequences.shape[0])
        emb = self._embed(sequences, device)
        return self.diffusion.inpaint(num_steps=timesteps, num_resamples=num_resamples, sampler=ADPM2Sampler(rho=1),
                                      sigma_schedule=KarrasSchedule(sigma_min=0.001, sigma_max=9.0, rho=3.0),
                                      inpaint=inpaint, in_paint_mask=in_paint_mask, embedding=emb,
                                      embedding_scale=cond_scale, draw=draw, seed=seed, sample0=sample0)

    def inpaint_tokens(self, sequences, device, draft_tokens, keep_mask, cond_scale=7.5, timesteps=100, num_resamples=1, *,
                       draw=None, seed=None, sample0=0, return_sample: bool = False):
        """inpaint() for a draft given as token ids, decoded: what inpaint_from_draft_and_conditioning does around
        model.inpaint (generative.py:1600-1614) -- the +-1 one-hot of the draft, the mask repeated over the channels, the
        argmax of the result -- inside the loop's own kernels (mdt_inpaint_enter / mdt_inpaint_finish), so neither the (B, C, L)
        source nor the full-shape mask is ever built.  ``draft_tokens``: integer (B, max_length), ids in [0, pred_dim);
        ``keep_mask``: bool (B, max_length), True = keep the position (the reference's in_paint_mask before its repeat).
        Returns (B, max_length) int64 token ids on ``device`` -- the draft id at a kept position -- and with ``return_sample``
        also the fp32 sample, bit for bit inpaint()'s on one_hot_draft(draft_tokens, pred_dim) and the repeated mask.
        ``cond_scale``: one guidance scale, or one per sample, as sample()."""
        draft_tokens, keep_mask = torch.as_tensor(draft_tokens), torch.as_tensor(keep_mask)
        B, L = sequences.shape[0], self.max_length
        cond_scale = guidance_rows(cond_scale, B)
        if draft_tokens.is_floating_point() or draft_tokens.is_complex() or draft_tokens.dtype == torch.bool:
            raise ValueError(f"draft_tokens must hold integer token ids, got {draft_tokens.dtype}")
        if keep_mask.dtype != torch.bool:
            raise ValueError(f"keep_mask must be a bool tensor (True = keep), got {keep_mask.dtype}")
        if tuple(draft_tokens.shape) != (B, L) or tuple(keep_mask.shape) != (B, L):
            raise ValueError(f"draft_tokens and keep_mask must be ({B}, {L}); got {tuple(draft_tokens.shape)} and "
                             f"{tuple(keep_mask.shape)}")
        device = torch.device(device)
        if B == 0:                                  # nothing to complete (sample() returns an empty tensor too)
            tok, x = torch.zeros(0, L, dtype=torch.int64, device=device), torch.empty(0, self.pred_dim, L, device=device)
            return (tok, x) if return_sample else tok
        lo, hi = (int(v) for v in torch.aminmax(draft_tokens))
        if lo < 0 or hi >= self.pred_dim:
            raise ValueError(f"draft_tokens holds ids in [{lo}, {hi}], the model has pred_dim = {self.pred_dim} classes")
        tok = torch.zeros(B, L, dtype=torch.int32, device=device)
        emb = self._embed(sequences, device)
        x = self.diffusion.inpaint(num_steps=timesteps, num_resamples=num_resamples, sampler=ADPM2Sampler(rho=1),
                                   sigma_schedule=KarrasSchedule(sigma_min=0.001, sigma_max=9.0, rho=3.0),
                                   inpaint=draft_tokens.to(device), in_paint_mask=keep_mask.to(device), embedding=emb,
                                   embedding_scale=cond_scale, draw=draw, seed=seed, sample0=sample0, tokens=tok)
        return (tok.long(), x) if return_sample else tok.long()

    # ------------------------------------------------------------------ refine: start from a lead, k per sample
    def _check_draft(self, draft_tokens, B: int) -> Tensor:
        """The draft of inpaint_tokens() / refine_tokens(): integer ids (B, max_length) in [0, pred_dim)."""
        draft_tokens = torch.as_tensor(draft_tokens)
        if draft_tokens.is_floating_point() or draft_tokens.is_complex() or draft_tokens.dtype == torch.bool:
            raise ValueError(f"draft_tokens must hold integer token ids, got {draft_tokens.dtype}")
        if tuple(draft_tokens.shape) != (B, self.max_length):
            raise ValueError(f"draft_tokens must be ({B}, {self.max_length}); got {tuple(draft_tokens.shape)}")
        if B:
            lo, hi = (int(v) for v in torch.aminmax(draft_tokens))
            if lo < 0 or hi >= self.pred_dim:
                raise ValueError(f"draft_tokens holds ids in [{lo}, {hi}], the model has pred_dim = {self.pred_dim} classes")
        return draft_tokens

    @staticmethod
    def _refine_sampler(sampler):
        """The sampler of a refine call (None: ADPM2Sampler(rho=1), sample()'s), which must have a fused kind."""
        if sampler is None:
            return ADPM2Sampler(rho=1)
        try:
            require_fused_kind(sampler)
        except TypeError:
            raise TypeError(f"{type(sampler).__name__}: refine() needs the fused loop (ADPM2Sampler, AEulerSampler or KarrasSampler "
                            "with the class's own step()): the start step enters inside the loop, which a per-step seam does not "
                            "have") from None
        return sampler

    def _check_keep(self, keep_mask, B: int, per_token_only: bool) -> Optional[Tensor]:
        """The keep mask of a refine call: None, or bool, True = keep -- (B, max_length), or (unless ``per_token_only``)
        (B, pred_dim, max_length)."""
        if keep_mask is None:
            return None
        keep_mask = torch.as_tensor(keep_mask)
        shapes = [(B, self.max_length)] + ([] if per_token_only else [(B, self.pred_dim, self.max_length)])
        if keep_mask.dtype != torch.bool:
            raise ValueError(f"keep_mask must be a bool tensor (True = keep), got {keep_mask.dtype}")
        if tuple(keep_mask.shape) not in shapes:
            raise ValueError(f"keep_mask must be {' or '.join(str(v) for v in shapes)}; got {tuple(keep_mask.shape)}")
        return keep_mask

    def _do_refine(self, sequences, device, start, cond_scale, timesteps, clamp, noise, sampler, sigma_schedule, trace=None,
                   source=None, draft=None, tokens=None, keep=None) -> Tensor:
        """refine() / refine_tokens() behind their checks: ``start`` and ``cond_scale`` are normalised (start_rows,
        guidance_rows), ``sampler`` has a fused kind (_refine_sampler), the batch is not empty.  The plain call -- seeded step noise, one guidance scale, no trace, token ids in
        and out -- is ONE custom op (mdt::refine_tokens; with a keep mask, checked by _check_keep, mdt::refine_keep_tokens);
        every other call is run_refine."""
        if sigma_schedule is None:
            sigma_schedule = KarrasSchedule(sigma_min=0.001, sigma_max=9.0, rho=3.0)
        device = torch.device(device)
        B = sequences.shape[0]
        emb = self._embed(sequences, device)
        eng = self.engine(device, emb.shape[1], B * (2 if is_guided(cond_scale) else 1))
        ns = self._noise_source(noise, B, device)
        kd = self.diffusion.diffusion
        sigmas = torch.as_tensor(sigma_schedule(timesteps, device), dtype=torch.float32).cpu()
        plain = (draft is not None and tokens is not None and ns.steps is None and trace is None and not clamp
                 and not isinstance(cond_scale, torch.Tensor) and any(type(sampler) is k.cls for k in FUSED_SAMPLERS.values()))
        if plain:
            rows = start if isinstance(start, torch.Tensor) else torch.full((B,), start, dtype=torch.int32)
            init = None if ns.init is None else ns.init.to(device=device, dtype=torch.float32)
            tail = (init, sigmas, ops.register_engine(eng), self.pred_dim, *ops.sampler_spec(sampler), float(kd.sigma_data),
                    float(cond_scale), int(ns.seed or 0), int(ns.sample0), float(kd.dynamic_threshold))
            if keep is None:
                x, t = torch.ops.mdt.refine_tokens(emb, draft.to(device), rows.to(device), *tail)
            else:
                x, t = torch.ops.mdt.refine_keep_tokens(emb, draft.to(device), rows.to(device), keep.to(device), *tail)
            tokens.copy_(t)
            return x
        with torch.no_grad():
            return run_refine(eng, emb, self.pred_dim, timesteps, ns, sigmas, sampler, kd.sigma_data, start, source=source,
                              draft=None if draft is None else draft.to(device), embedding_scale=cond_scale, clamp=clamp,
                              trace=trace, tokens=tokens, dynamic_threshold=float(kd.dynamic_threshold),
                              keep=None if keep is None else keep.to(device), keep_per_token=keep is not None and keep.dim() == 2)

    def refine(self, sequences, device, source, start_step, cond_scale=None, timesteps=100, clamp=False, *, noise=None,
               sampler=None, sigma_schedule=None, trace=None):
        """Partial-noise editing (the k-diffusion form): noise ``source`` -- fp32 (B, pred_dim, max_length), e.g.
        one_hot_draft(tokens, pred_dim) -- up to the level of timestep ``start_step`` of the schedule,
        ``x = source + sigmas[k] * randn_like(source)`` (the expression of diffusion.py:535), and run the remaining
        ``timesteps - 1 - k`` sampler steps under the conditioning.  A small k (much noise) gives far-away results, a large k near
        ones; a zero source at k = 0 is sample().

        ``start_step``: one int in [0, timesteps - 2], or one per sample (a 1-D list / tuple / ndarray / integer tensor of B
        entries, diffusion.start_rows): row b is then row b of the call at start_step[b], bit for bit under a pinned
        ``kernel_choice``.  Cost: a per-sample call runs EVERY row from min(start_step) -- rows that start later ride along
        until their step -- so it costs what the scalar call at min(start_step) costs.  ``cond_scale`` (None: sample()'s default),
        ``noise`` (a tensor = the entry noise, a NoiseSource, or None), ``sampler``, ``sigma_schedule``, ``trace``, ``clamp`` as
        sample().  The sampler must have a fused loop: a sampler with its own step() raises TypeError.  Every position is free;
        refine_keep() holds a scaffold fixed."""
        return self.refine_keep(sequences, device, source, start_step, cond_scale, timesteps, clamp, noise=noise, sampler=sampler,
                                sigma_schedule=sigma_schedule, trace=trace)

    def refine_keep(self, sequences, device, source, start_step, cond_scale=None, timesteps=100, clamp=False, *, noise=None,
                    sampler=None, sigma_schedule=None, trace=None, keep_mask=None):
        """refine() around a kept scaffold: every argument as refine(), and ``keep_mask`` (bool, True = keep; (B, pred_dim,
        max_length) or (B, max_length); None: refine() itself).  The kept positions are re-noised from ``source`` in front of
        every step, as ADPM2Sampler.inpaint does, and equal ``source`` exactly in the result (before ``clamp``); the free
        positions start from the noised source, not from pure noise.  With start_step = 0 this is scaffold-constrained
        generation under any fused sampler.  No resamples.  An all-False mask is refine(), bit for bit.  Explicit noise needs
        NoiseSource(sources=...).  Cost: one more elementwise launch per step, and EVERY row runs from min(start_step)."""
        sampler = self._refine_sampler(sampler)
        if cond_scale is None:
            cond_scale = 7.5 if self._inverse else 1.0
        B = sequences.shape[0]
        cond_scale = guidance_rows(cond_scale, B)
        start = start_rows(start_step, B, timesteps)
        source = torch.as_tensor(source)
        if not source.is_floating_point() or tuple(source.shape) != (B, self.pred_dim, self.max_length):
            raise ValueError(f"source must be a floating-point tensor ({B}, {self.pred_dim}, {self.max_length}); got {source.dtype} "
                             f"{tuple(source.shape)}")
        keep = self._check_keep(keep_mask, B, per_token_only=False)
        if B == 0:
            return torch.empty(0, self.pred_dim, self.max_length, device=torch.device(device))
        return self._do_refine(sequences, device, start, cond_scale, timesteps, clamp, noise, sampler, sigma_schedule, trace,
                               source=source, keep=keep)

    def refine_tokens(self, sequences, device, draft_tokens, start_step=None, *, strength=None, cond_scale=None, timesteps=100,
                      noise=None, sampler=None, sigma_schedule=None, return_sample: bool = False):
        """refine() for a lead given as token ids, decoded: the +-1 one-hot of the draft and the argmax of the result live inside
        the loop's own kernels (mdt_refine_enter, the last update kernel), so the (B, C, L) source is never built.
        ``draft_tokens``: integer (B, max_length), ids in [0, pred_dim).  Give exactly one of ``start_step`` (as refine()) or
        ``strength`` in (0, 1] (diffusion.refine_start; one value or one per sample): the share of the schedule that is run.
        Returns (B, max_length) int64 token ids on ``device`` and with ``return_sample`` also the fp32 sample, bit for bit
        refine()'s on one_hot_draft(draft_tokens, pred_dim).  Cost of a per-sample call: every row runs from min(start_step).
        Every position is free; refine_keep_tokens() holds a scaffold fixed."""
        return self.refine_keep_tokens(sequences, device, draft_tokens, start_step, strength=strength, cond_scale=cond_scale,
                                       timesteps=timesteps, noise=noise, sampler=sampler, sigma_schedule=sigma_schedule,
                                       return_sample=return_sample)

    def refine_keep_tokens(self, sequences, device, draft_tokens, start_step=None, *, strength=None, cond_scale=None,
                           timesteps=100, noise=None, sampler=None, sigma_schedule=None, return_sample: bool = False,
                           keep_mask=None):
        """refine_tokens() around a kept scaffold (refine_keep() for a lead given as token ids): every argument as
        refine_tokens(), and ``keep_mask``: bool (B, max_length), True = keep the position, as inpaint_tokens() (None:
        refine_tokens() itself).  The scaffold is held exactly -- a kept position decodes to its draft id -- while the rest is
        refined near the lead."""
        sampler = self._refine_sampler(sampler)
        if (start_step is None) == (strength is None):
            raise ValueError("give exactly one of start_step and strength")
        if strength is not None:
            start_step = refine_start(timesteps, strength)
        if cond_scale is None:
            cond_scale = 7.5 if self._inverse else 1.0
        B, L = sequences.shape[0], self.max_length
        cond_scale = guidance_rows(cond_scale, B)
        start = start_rows(start_step, B, timesteps, "start_step" if strength is None else "strength")
        draft_tokens = self._check_draft(draft_tokens, B)
        keep = self._check_keep(keep_mask, B, per_token_only=True)
        device = torch.device(device)
        if B == 0:                                  # nothing to refine (sample() returns an empty tensor too)
            tok, x = torch.zeros(0, L, dtype=torch.int64, device=device), torch.empty(0, self.pred_dim, L, device=device)
            return (tok, x) if return_sample else tok
        tok = torch.zeros(B, L, dtype=torch.int32, device=device)
        x = self._do_refine(sequences, device, start, cond_scale, timesteps, False, noise, sampler, sigma_schedule,
                            draft=draft_tokens, tokens=tok, keep=keep)
        return (tok.long(), x) if return_sample else tok.long()


class QMDiffusion(_QMBase):
    """Generative inverse diffusion model (generative.py:718-914)."""

    _inverse = True

    def __init__(self, max_length=1024, channels=128, pred_dim=1, context_embedding_max_length=32, unet_type="cfg",
                 pos_emb_fourier=True, pos_emb_fourier_add=False, text_embed_dim=1024, embed_dim_position=64,
                 unet=None):
        super().__init__()
        print("Using unet type: ", unet_type)
        self._init_common(max_length, channels, pred_dim, unet, context_embedding_max_length, unet_type,
                          pos_emb_fourier, pos_emb_fourier_add, text_embed_dim, embed_dim_position)

    def sample(self, sequences, device, cond_scale=7.5, timesteps=100, clamp=False, *, noise=None, trace=None,
               timer=None, sampler=None, sigma_schedule=None):
        """``sampler``: ADPM2Sampler(rho=1) (None, the reference's choice), AEulerSampler() -- one U-Net evaluation per
        timestep instead of two -- KarrasSampler(...) or any Sampler; ``sigma_schedule``: KarrasSchedule(0.001, 9.0, 3.0) (None)
        or any callable (num_steps, device) -> sigmas."""
        return self._do_sample(sequences, device, cond_scale, timesteps, clamp, noise, trace, timer, sampler=sampler,
                               sigma_schedule=sigma_schedule)


class QMDiffusionForward(_QMBase):
    """Forward diffusion property predictor (generative.py:31-225); note `unet` is the 4th positional."""

    _inverse = False

    def __init__(self, max_length=1024, channels=128, pred_dim=1, unet=None, context_embedding_max_length=32,
                 unet_type="cfg", pos_emb_fourier=True, pos_emb_fourier_add=False, text_embed_dim=1024,
                 embed_dim_position=64):
        super().__init__()
        self._init_common(max_length, channels, pred_dim, unet, context_embedding_max_length, unet_type,
                          pos_emb_fourier, pos_emb_fourier_add, text_embed_dim, embed_dim_position)

    def sample(self, sequences, device, cond_scale=1.0, timesteps=100, clamp=False, *, noise=None, trace=None,
               timer=None, sampler=None, sigma_schedule=None):
        """``sampler``: ADPM2Sampler(rho=1) (None, the reference's choice), AEulerSampler() -- one U-Net evaluation per
        timestep instead of two -- KarrasSampler(...) or any Sampler; ``sigma_schedule``: KarrasSchedule(0.001, 9.0, 3.0) (None)
        or any callable (num_steps, device) -> sigmas."""
        return self._do_sample(sequences, device, cond_scale, timesteps, clamp, noise, trace, timer, sampler=sampler,
                               sigma_schedule=sigma_schedule)


# ----------------------------------------------------------------------------------------------------------------------
# the inverse -> forward validation chain of the reference's callers, kept on the device
# ----------------------------------------------------------------------------------------------------------------------
def tokens_to_forward_input(tokens: Tensor, max_length: int, X_norm_factor: float = 1.0) -> Tensor:
    """What the reference does between the two models with strings (generative.py:1229 reverse_tokenize ->
    predict_properties_from_SMILES :425-429 texts_to_sequences + pad_sequences(maxlen, padding='post',
    truncating='post') / X_norm_factor), restated on token ids: id 0 is "no character" (keras' sequences_to_texts skips
    it), so every row is compacted to its non-zero ids in order, truncated / zero-padded at the end to ``max_length`` and
    scaled.  Assumes every id 1..pred_dim-1 is in the tokenizer's vocabulary (as produced by the one-hot training data).
    Pinned bit for bit by tests/golden/token_chain.npz (the reference's own two functions over a restated keras tokenizer)."""
    tok = tokens.long()
    B, L = tok.shape
    keep = tok != 0
    order = torch.argsort((~keep).to(torch.int8), dim=1, stable=True)          # non-zero ids first, original order kept
    packed = torch.gather(tok * keep, 1, order)
    out = torch.zeros(B, max_length, dtype=torch.float64, device=tok.device)
    n = min(L, max_length)
    out[:, :n] = packed[:, :n].double()
    # the reference divides the int32 array by X_norm_factor in float64 (numpy) and torch.Tensor() rounds to fp32 (generative.py:428-429)
    return (out / X_norm_factor).float()


def predict_properties_from_tokens(model_forward: "QMDiffusionForward", tokens: Tensor, device, cond_scale: float = 1.0,
                                   timesteps: int = 100, clamp: bool = False, X_norm_factor: float = 1.0,
                                   context_embedding_max_length: int = 12, noise=None, *, sampler=None,
                                   sigma_schedule=None) -> Tensor:
    """predict_properties_from_SMILES (generative.py:404-451) for molecules given as token ids on the device: the forward
    model's sample() on the re-tokenised ids, first ``context_embedding_max_length`` positions = the (scaled) properties.
    Returns (B, context_embedding_max_length) on ``device`` (the caller applies scaler.inverse_transform)."""
    data = tokens_to_forward_input(tokens.to(device), model_forward.max_length, X_norm_factor)
    result = model_forward.sample(data, device, cond_scale=cond_scale, timesteps=timesteps, clamp=clamp, noise=noise,
                                  sampler=sampler, sigma_schedule=sigma_schedule)
    return result[:, 0, :context_embedding_max_length]


def generate_and_validate(model: "QMDiffusion", model_forward: "QMDiffusionForward", conditioning: Tensor, device,
                          cond_scale: float = 1.0, timesteps: int = 100, forward_timesteps: int = 100,
                          X_norm_factor: float = 1.0, noise=None, forward_noise=None, *, sampler=None, sigma_schedule=None):
    """generate_from_conditioning's core (generative.py:1685-1713) without leaving the GPU: sample molecules for the
    conditioning, decode them inside the last sampler update, re-predict their properties with the forward model.
    Returns (tokens (B, L) int64, predicted properties (B, n_cond))."""
    tokens = model.sample_tokens(conditioning, device, cond_scale=cond_scale, timesteps=timesteps, noise=noise,
                                 sampler=sampler, sigma_schedule=sigma_schedule)
    props = predict_properties_from_tokens(model_forward, tokens, device, cond_scale=1.0, timesteps=forward_timesteps,
                                           X_norm_factor=X_norm_factor,
                                           context_embedding_max_length=conditioning.shape[1], noise=forward_noise,
                                           sampler=sampler, sigma_schedule=sigma_schedule)
    return tokens, props


def guidance_sweep(model, sequences: Tensor, cond_scales, device, *, tokens: bool = False, **sample_kwargs):
    """The guidance sweep of the reference's callers -- ``for s in cond_scales: model.sample(sequences, device, cond_scale=s)``
    (sample_loop_generative, generative.py:1206) -- as ONE fused call of batch S * B: row s * B + b is conditioning b at
    cond_scales[s], and the result comes back as (S, B, ...).  ``tokens``: one sample_tokens() call instead of one sample() call
    (token ids (S, B, L); with return_sample=True the pair of ids and samples).  ``sample_kwargs`` go to that call; a ``noise``
    tensor holds S * B rows, and with ``noise=NoiseSource(seed=..., sample0=n)`` sweep s equals the scalar call whose sample0 is
    n + s * B (bit for bit under a pinned ``kernel_choice``)."""
    try:
        ndim = torch.as_tensor(cond_scales).dim()
    except Exception:
        ndim = -1
    if ndim != 1:
        raise ValueError("cond_scales must be a 1-D sequence of guidance scales, one per sweep")
    S, B = len(cond_scales), sequences.shape[0]
    scales = torch.as_tensor(guidance_rows(cond_scales, S, "cond_scales"), dtype=torch.float32).reshape(-1).expand(S)
    call = model.sample_tokens if tokens else model.sample
    out = call(sequences.repeat(S, *([1] * (sequences.dim() - 1))), device, cond_scale=scales.repeat_interleave(B), **sample_kwargs)
    unflat = lambda t: t.reshape(S, B, *t.shape[1:])          # noqa: E731
    return tuple(unflat(t) for t in out) if isinstance(out, tuple) else unflat(out)


# ----------------------------------------------------------------------------------------------------------------------
# the draft-completion chain of the reference's callers (inpaint_from_draft_and_conditioning), kept on the device
# ----------------------------------------------------------------------------------------------------------------------
def one_hot_draft(tokens: Tensor, num_classes: int) -> Tensor:
    """The tensor half of encode_SMILES_into_one_hot (generative.py:1567-1569) and the permute of its caller (:1603): token ids
    (B, L) -> fp32 (B, num_classes, L) with +1 at the id's channel and -1 elsewhere.  What the dense inpaint() takes as
    ``inpaint``; inpaint_tokens() never builds it."""
    tok = torch.as_tensor(tokens).long()
    cls = torch.arange(num_classes, device=tok.device).view(1, num_classes, 1)
    return torch.where(tok.unsqueeze(1) == cls, 1.0, -1.0).to(torch.float32)


def complete_and_validate(model: "QMDiffusion", model_forward: "QMDiffusionForward", conditioning: Tensor, draft_tokens: Tensor,
                          keep_mask: Tensor, device, cond_scale: float = 1.0, timesteps: int = 100,
                          forward_timesteps: int = 100, num_resamples: int = 1, X_norm_factor: float = 1.0, forward_noise=None, *,
                          draw=None, seed=None, sample0: int = 0):
    """inpaint_from_draft_and_conditioning's core (generative.py:1600-1660) without leaving the GPU: complete the draft under
    the conditioning -- kept positions stay, the rest is regenerated -- decode inside the loop's last kernel, re-predict the
    properties of the completed molecules with the forward model.  Returns (tokens (B, L) int64, predicted properties
    (B, n_cond)).  ``draw`` / ``seed`` / ``sample0`` as inpaint_tokens; ``forward_noise`` as generate_and_validate."""
    tokens = model.inpaint_tokens(conditioning, device, draft_tokens, keep_mask, cond_scale=cond_scale, timesteps=timesteps,
                                  num_resamples=num_resamples, draw=draw, seed=seed, sample0=sample0)
    props = predict_properties_from_tokens(model_forward, tokens, device, cond_scale=1.0, timesteps=forward_timesteps,
                                           X_norm_factor=X_norm_factor,
                                           context_embedding_max_length=conditioning.shape[1], noise=forward_noise)
    return tokens, props


# ----------------------------------------------------------------------------------------------------------------------
# lead refinement: explore the neighbourhood of a draft under new target properties
# ----------------------------------------------------------------------------------------------------------------------
def strength_sweep(model, sequences: Tensor, draft_tokens: Tensor, strengths, device, **refine_kwargs):
    """The strength sweep over the same leads -- ``for s in strengths: model.refine_tokens(sequences, device, draft_tokens,
    strength=s)`` -- as ONE fused call of batch S * B, the counterpart of guidance_sweep: row s * B + b is lead b at strengths[s],
    and the token ids come back as (S, B, L) (with return_sample=True the pair of ids and samples (S, B, C, L)).
    ``refine_kwargs`` go to refine_tokens() -- with a ``keep_mask`` (B, L), the same scaffold at every strength, to
    refine_keep_tokens(); a ``noise`` tensor holds S * B rows, and with ``noise=NoiseSource(seed=..., sample0=n)``
    sweep s equals the scalar call whose sample0 is n + s * B (bit for bit under a pinned ``kernel_choice``).  Cost: every row runs
    from the start step of the LARGEST strength, so the sweep pays off only while its scalar calls underfill the GPU."""
    try:
        ndim = torch.as_tensor(strengths).dim()
    except Exception:
        ndim = -1
    if ndim != 1 or len(strengths) == 0:
        raise ValueError("strengths must be a non-empty 1-D sequence, one strength per sweep")
    if "start_step" in refine_kwargs or "strength" in refine_kwargs:
        raise ValueError("strength_sweep sets the start steps itself: give strengths, not start_step / strength")
    S, B = len(strengths), sequences.shape[0]
    starts = refine_start(int(refine_kwargs.get("timesteps", 100)), strengths)
    draft_tokens = torch.as_tensor(draft_tokens)
    call = model.refine_tokens
    if refine_kwargs.get("keep_mask") is not None:            # the same scaffold at every strength
        refine_kwargs["keep_mask"] = torch.as_tensor(refine_kwargs["keep_mask"]).repeat(S, 1)
        call = model.refine_keep_tokens
    else:
        refine_kwargs.pop("keep_mask", None)
    out = call(sequences.repeat(S, *([1] * (sequences.dim() - 1))), device, draft_tokens.repeat(S, 1),
               start_step=torch.tensor(starts, dtype=torch.int64).repeat_interleave(B), **refine_kwargs)
    unflat = lambda t: t.reshape(S, B, *t.shape[1:])          # noqa: E731
    return tuple(unflat(t) for t in out) if isinstance(out, tuple) else unflat(out)


def refine_and_validate(model: "QMDiffusion", model_forward: "QMDiffusionForward", conditioning: Tensor, draft_tokens: Tensor,
                        device, start_step=None, *, strength=None, cond_scale: float = 1.0, timesteps: int = 100,
                        forward_timesteps: int = 100, X_norm_factor: float = 1.0, noise=None, forward_noise=None, sampler=None,
                        sigma_schedule=None, keep_mask=None):
    """The chain into the forward model, as complete_and_validate: refine the leads under the conditioning, decode inside the
    last sampler update, re-predict the properties of the refined molecules with the forward model.  Returns (tokens (B, L)
    int64, predicted properties (B, n_cond)).  ``start_step`` / ``strength`` / ``noise`` as refine_tokens, ``keep_mask``
    as refine_keep_tokens; ``forward_noise`` as generate_and_validate."""
    call, more = (model.refine_tokens, {}) if keep_mask is None else (model.refine_keep_tokens, dict(keep_mask=keep_mask))
    tokens = call(conditioning, device, draft_tokens, start_step, strength=strength, cond_scale=cond_scale, timesteps=timesteps,
                  noise=noise, sampler=sampler, sigma_schedule=sigma_schedule, **more)
    props = predict_properties_from_tokens(model_forward, tokens, device, cond_scale=1.0, timesteps=forward_timesteps,
                                           X_norm_factor=X_norm_factor,
                                           context_embedding_max_length=conditioning.shape[1], noise=forward_noise)
    return tokens, props


# ----------------------------------------------------------------------------------------------------------------------
# screening: the best distinct, novel molecules out of N tries per target, on the device (csrc/k_screen.hip)
# ----------------------------------------------------------------------------------------------------------------------
MAX_CANDIDATES = 1024           # mdt_screen_select's limits (include/mdt_hip.h)
MAX_SCREEN_LENGTH = 1024
MAX_SCREEN_PROPERTIES = 64
MAX_EDIT_LENGTH = 64            # the edit distance (csrc/k_edit.hip): one 64-bit word per row, one mask per id
MAX_EDIT_ID = 64
MAX_MOL_LENGTH = 64             # the molecular graph and its key (csrc/k_molgraph.hip): at most 64 atoms, one root per lane
MAX_WRITE_WIDTH = rt.MOLW_MAX_WIDTH    # the SMILES writer (csrc/k_molwrite.hip): written rows of at most 128 tokens
IDENTITIES = ("string", "graph")
FP_SIM_DEN = 65536              # a similarity threshold crosses into the kernels as sim_num / 65536 (MDT_FP_SIM_DEN)
MAX_SUB_PATTERNS = 32           # the substructure match (csrc/k_molsub.hip): patterns a call, one bit of a 32-bit word each
MAX_SUB_LENGTH = 32             # ... and characters a pattern
MAX_FP_RADIUS = 3               # the fingerprint (csrc/k_molfp.hip): rounds 0 .. radius, radius in [0, 3]
MOLH_MAX_STEPS = 4096           # the Kekule check (csrc/k_molh.hip): tries of a row's matching search (MDT_MOLH_MAX_STEPS)


def _integer_ids(ids, name: str):
    """``ids`` as a numpy array (host data) or a tensor, refused unless its dtype is an integer one."""
    import numpy as np
    if not isinstance(ids, Tensor):
        ids = np.asarray(ids)
        if ids.dtype.kind not in "iu":
            raise ValueError(f"{name} must hold integer token ids, got dtype {ids.dtype}")
    elif ids.dtype == torch.bool or ids.is_floating_point() or ids.is_complex():
        raise ValueError(f"{name} must hold integer token ids, got dtype {ids.dtype}")
    if ids.ndim != 2:
        raise ValueError(f"{name} must be 2-D (rows, positions), got shape {tuple(ids.shape)}")
    return ids


def token_keys(packed, length):
    """The 64-bit key of mdt_tokens_compact (include/mdt_hip.h) on the host: numpy uint64 (M,) for left-packed rows (M, L) and
    their lengths -- the sum mod 2^64 over j < length of one splitmix64 step of (j << 32) | uint32(id)."""
    import numpy as np
    packed = np.asarray(packed).astype(np.int64)
    M, L = packed.shape
    j = np.arange(L, dtype=np.uint64)[None, :]
    with np.errstate(over="ignore"):
        z = ((j << np.uint64(32)) | (packed & 0xFFFFFFFF).astype(np.uint64)) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
        z = np.where(j < np.asarray(length).astype(np.uint64)[:, None], z, np.uint64(0))
        return z.sum(axis=1, dtype=np.uint64)


class KnownSet:
    """The molecules a generated one is "novel" against (ALL_SMILES of is_novel, generative.py:1063), as token ids: built once on the
    host from (M, L_any) integer ids -- the training set through the tokenizer -- for generated rows of ``length`` positions.

    Every row is compacted (non-zero ids in order: the string of the character-level tokenizer, which skips id 0); rows with more
    than ``length`` non-zero ids are dropped (they equal no generated molecule), exact duplicates are dropped, and the rest is sorted
    by the key of mdt_tokens_compact (stable).  ``packed`` int32 (M, length), ``lengths`` int32 (M), ``key`` uint64 (M), numpy.
    The device copy is made on first use and cached, one per device."""

    def __init__(self, tokens, length: int):
        import numpy as np
        if isinstance(length, bool) or not isinstance(length, int) or not 1 <= length <= MAX_SCREEN_LENGTH:
            raise ValueError(f"length must be an int in [1, {MAX_SCREEN_LENGTH}], got {length!r}")
        ids = _integer_ids(tokens, "known_tokens")
        ids = (ids.detach().cpu().numpy() if isinstance(ids, Tensor) else ids).astype(np.int64)
        M, L = ids.shape
        order = np.argsort(ids == 0, axis=1, kind="stable")                  # non-zero ids first, original order kept
        packed = np.take_along_axis(ids, order, axis=1)
        n = (ids != 0).sum(axis=1)
        packed = packed[n <= length]
        wide = np.zeros((packed.shape[0], max(L, length)), dtype=np.int64)
        wide[:, :L] = packed
        packed = np.unique(wide[:, :length], axis=0) if len(wide) else wide[:, :length]
        lengths = (packed != 0).sum(axis=1)
        key = token_keys(packed, lengths)
        by_key = np.argsort(key, kind="stable")
        self.width = length
        self.packed = np.ascontiguousarray(packed[by_key].astype(np.int32))
        self.lengths = np.ascontiguousarray(lengths[by_key].astype(np.int32))
        self.key = np.ascontiguousarray(key[by_key])
        self._on = {}
        self._mol_keys = {}
        self._fingerprints = {}
        self._scaffold_keys = {}
        self._id_range = None

    def __len__(self) -> int:
        return int(self.key.shape[0])

    def on(self, device):
        """(key int64: the uint64 bits, packed int32 (M, length), lengths int32 (M)) on ``device``."""
        import numpy as np
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._on:
            self._on[device] = (torch.from_numpy(self.key.view(np.int64)).to(device), torch.from_numpy(self.packed).to(device),
                                torch.from_numpy(self.lengths).to(device))
        return self._on[device]

    def mol_keys(self, vocabulary: "SmilesVocabulary", device, *, normalize: bool = False) -> Tensor:
        """The graph keys of the known molecules (mol_key()): int64 (M',) on ``device`` holding the uint64 bits of the sorted unique
        NON-ZERO keys of the known rows -- rows that are no molecule under ``vocabulary`` (key 0) drop out, respellings of one
        molecule count once.  Computed once by mdt::mol_graph -> mdt::mol_key and cached per (vocabulary, device).  Sorted ascending
        AS UNSIGNED, which is what mdt::key_flags' binary search needs: on int64 storage that is a signed sort of (key ^ 2^63) --
        flipping the top bit maps unsigned order onto signed order -- flipped back afterwards.  ``width`` > 64 raises ValueError.
        ``normalize=True``: the keys of the normal forms (mol_normalize(): mdt::mol_hydrogens -> mdt::mol_rings ->
        mdt::mol_normalize between the two launches), cached apart from the keys as written."""
        _normalize_arg(normalize)
        if not isinstance(vocabulary, SmilesVocabulary):
            raise ValueError(f"vocabulary must be a SmilesVocabulary, got {type(vocabulary).__name__}")
        if self.width > MAX_MOL_LENGTH:
            raise ValueError(f"known_tokens has rows of {self.width} positions; the graph key takes at most {MAX_MOL_LENGTH} "
                             "(wider rows are out of scope)")
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        at = (id(vocabulary), device, normalize)
        if at not in self._mol_keys:
            _, packed, lengths = self.on(device)
            graph, _, _ = _graph_rows(packed, lengths, vocabulary, device, normalize)
            key = torch.ops.mdt.mol_key(*graph)
            top = -2 ** 63                                                     # the bit pattern 1 << 63
            key = torch.unique(key[key != 0] ^ top) ^ top                      # unique() sorts ascending (signed)
            self._mol_keys[at] = (vocabulary, key)                             # (the vocabulary is held: its id stays its own)
        return self._mol_keys[at][1]

    def fingerprints(self, vocabulary: "SmilesVocabulary", device, radius: int = 2, *, normalize: bool = False):
        """The fingerprints of the known molecules (mol_fingerprint()): (fp int64 (M, 16): the uint64 bits, count int32 (M,)) on
        ``device`` for ALL rows of ``packed``, in that order, so an index into them is an index into ``packed``.  Rows that are no
        molecule under ``vocabulary`` have an all-zero fingerprint (similarity 0 to everything).  Computed once by mdt::mol_graph ->
        mdt::mol_fp and cached per (vocabulary, device, radius).  ``width`` > 64 raises ValueError.  ``normalize=True``: the
        fingerprints of the normal forms (mol_normalize()), cached apart from those of the rows as written."""
        _normalize_arg(normalize)
        if not isinstance(vocabulary, SmilesVocabulary):
            raise ValueError(f"vocabulary must be a SmilesVocabulary, got {type(vocabulary).__name__}")
        if self.width > MAX_MOL_LENGTH:
            raise ValueError(f"known_tokens has rows of {self.width} positions; the fingerprint takes at most {MAX_MOL_LENGTH} "
                             "(wider rows are out of scope)")
        radius = _radius_arg(radius)
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        at = (id(vocabulary), device, radius, normalize)
        if at not in self._fingerprints:
            _, packed, lengths = self.on(device)
            graph, _, _ = _graph_rows(packed, lengths, vocabulary, device, normalize)
            self._fingerprints[at] = (vocabulary, torch.ops.mdt.mol_fp(*graph, radius))
        return self._fingerprints[at][1]

    def scaffold_keys(self, vocabulary: "SmilesVocabulary", device, *, normalize: bool = False, exocyclic: bool = True,
                      generic: bool = False) -> Tensor:
        """The scaffold keys of the known molecules (scaffold_key()): int64 (M',) on ``device`` holding the uint64 bits of the sorted
        unique NON-ZERO keys -- rows that are no molecule and acyclic molecules (no scaffold: key 0) drop out, all decorations of one
        ring framework count once.  Sorted ascending AS UNSIGNED, as mol_keys() and for the same reader (mdt::key_flags).  Computed
        once by mdt::mol_graph -> mdt::mol_scaffold -> mdt::mol_key (``normalize=True``: the three launches of the normal form
        after the first) and cached per (vocabulary, device, normalize, exocyclic, generic).  ``width`` > 64 raises ValueError."""
        _normalize_arg(normalize)
        mode = _scaffold_mode(exocyclic, generic)
        if not isinstance(vocabulary, SmilesVocabulary):
            raise ValueError(f"vocabulary must be a SmilesVocabulary, got {type(vocabulary).__name__}")
        if self.width > MAX_MOL_LENGTH:
            raise ValueError(f"known_tokens has rows of {self.width} positions; the scaffold takes at most {MAX_MOL_LENGTH} "
                             "(wider rows are out of scope)")
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        at = (id(vocabulary), device, normalize, exocyclic, generic)
        if at not in self._scaffold_keys:
            _, packed, lengths = self.on(device)
            graph, _, _ = _graph_rows(packed, lengths, vocabulary, device, normalize)
            key = torch.ops.mdt.mol_key(*torch.ops.mdt.mol_scaffold(*graph, mode)[:4])
            top = -2 ** 63                                                     # the bit pattern 1 << 63
            key = torch.unique(key[key != 0] ^ top) ^ top                      # unique() sorts ascending (signed)
            self._scaffold_keys[at] = (vocabulary, key)                        # (the vocabulary is held: its id stays its own)
        return self._scaffold_keys[at][1]

    def id_range(self):
        """(lowest, highest) id of the set, looked up once on the host arrays; (0, 0) for an empty set."""
        if self._id_range is None:
            self._id_range = (int(self.packed.min()), int(self.packed.max())) if self.packed.size else (0, 0)
        return self._id_range


class Screened(NamedTuple):
    """screen_tokens' result, G groups (targets), K = ``keep`` slots per group in ascending order of score."""
    tokens: Tensor     # (G, K, L) int64: the kept candidates' ids as they were given; 0 in unfilled slots
    props: Tensor      # (G, K, n): their re-predicted (scaled) properties; NaN in unfilled slots
    score: Tensor      # (G, K): the weighted mean squared distance from the target; +inf in unfilled slots
    index: Tensor      # (G, K) int64: the candidate c (row c * G + g of the input); -1 in unfilled slots
    count: Tensor      # (G,) int64: filled slots = min(K, eligible candidates)
    status: Tensor     # (N, G) uint8: 1 empty | 2 non-finite score | 4 duplicate of a lower c | 8 in the known set (or closer to
    #                    it than min_novelty) | 16 closer than min_distance to a better kept candidate (screen_tokens_diverse)
    #                    | 32 malformed | 64 overvalent (with ``vocabulary=``: smiles_check's verdict; never kept)


def _screen_args(conditioning, candidates, keep, known_tokens, weights, tokens=None, length=None):
    """Every refusal of screen_tokens / screen_candidates, before anything is launched.  Returns (weights fp32 CPU or None,
    KnownSet or None)."""
    for name, v in (("candidates", candidates), ("keep", keep)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"{name} must be an int, got {v!r}")
    if not 1 <= candidates <= MAX_CANDIDATES:
        raise ValueError(f"candidates must lie in [1, {MAX_CANDIDATES}], got {candidates}")
    if not 1 <= keep <= candidates:
        raise ValueError(f"keep must lie in [1, candidates = {candidates}], got {keep}")
    if not isinstance(conditioning, Tensor) or conditioning.dim() != 2:
        raise ValueError("conditioning must be a 2-D tensor (G, n): one target per group")
    G, n = conditioning.shape
    if not 1 <= n <= MAX_SCREEN_PROPERTIES:
        raise ValueError(f"conditioning must hold 1 to {MAX_SCREEN_PROPERTIES} properties per target, got {n}")
    if tokens is not None:
        tokens = _integer_ids(tokens, "tokens")
        if tokens.shape[0] != candidates * G:
            raise ValueError(f"tokens must hold candidates * G = {candidates * G} rows (row c * G + g), got {tokens.shape[0]}")
        length = tokens.shape[1]
    if not 1 <= length <= MAX_SCREEN_LENGTH:
        raise ValueError(f"tokens must hold 1 to {MAX_SCREEN_LENGTH} positions per row, got {length}")
    if weights is not None:
        try:
            weights = torch.as_tensor(weights).detach().to(device="cpu", dtype=torch.float32)
        except Exception as e:
            raise ValueError(f"weights must hold one number per property ({e})") from None
        if tuple(weights.shape) != (n,):
            raise ValueError(f"weights must hold one value per property ({n}), got shape {tuple(weights.shape)}")
        if not bool(torch.isfinite(weights).all()) or bool((weights < 0).any()):
            raise ValueError("weights must be finite and not negative")
    if known_tokens is not None and not isinstance(known_tokens, KnownSet):
        known_tokens = KnownSet(known_tokens, length)
    if known_tokens is not None and known_tokens.width != length:
        raise ValueError(f"known_tokens was built for rows of {known_tokens.width} positions, tokens has {length}")
    return weights, known_tokens


def _edit_width(length: int, what: str) -> None:
    if length > MAX_EDIT_LENGTH:
        raise ValueError(f"{what} has rows of {length} positions; the edit distance takes at most {MAX_EDIT_LENGTH} "
                         "(multi-word rows are out of scope)")


def _edit_ids(ids, what: str):
    """Refuses ids outside [0, MAX_EDIT_ID): one aminmax, the one host synchronisation of the edit-distance paths."""
    t = torch.as_tensor(ids)
    if t.numel():
        lo, hi = (int(v) for v in torch.aminmax(t))
        if lo < 0 or hi >= MAX_EDIT_ID:
            raise ValueError(f"{what} holds ids from {lo} to {hi}; the edit distance takes ids in [0, {MAX_EDIT_ID})")
    return t


def _edit_known(known: "KnownSet") -> None:
    lo, hi = known.id_range()
    if lo < 0 or hi >= MAX_EDIT_ID:
        raise ValueError(f"known_tokens holds ids from {lo} to {hi}; the edit distance takes ids in [0, {MAX_EDIT_ID})")


def _diverse_args(min_distance, min_novelty, known, length=None, tokens=None) -> bool:
    """The refusals of the two edit-distance filters, before anything is launched; ``length`` or the ``tokens`` themselves, as
    _screen_args.  -> whether either filter is on (if neither is, nothing is looked at)."""
    for name, v in (("min_distance", min_distance), ("min_novelty", min_novelty)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError(f"{name} must be an int >= 1, got {v!r}")
    if min_distance == 1 and min_novelty == 1:
        return False
    if tokens is not None:
        tokens = torch.as_tensor(tokens)
        length = tokens.shape[1]
    _edit_width(length, "tokens")
    if min_novelty > 1:
        if known is None or len(known) == 0:
            raise ValueError(f"min_novelty = {min_novelty} asks for the distance to the known set: give a non-empty known_tokens")
        _edit_known(known)
    if tokens is not None:
        _edit_ids(tokens, "tokens")
    return True


def _radius_arg(radius) -> int:
    if isinstance(radius, bool) or not isinstance(radius, int) or not 0 <= radius <= MAX_FP_RADIUS:
        raise ValueError(f"the fingerprint radius must be an int in [0, {MAX_FP_RADIUS}], got {radius!r}")
    return radius


def _similarity_args(max_similarity, max_known_similarity, fingerprint_radius, vocabulary, known, length: int):
    """The refusals of the two similarity thresholds, before anything is launched.  -> (sim_num or None, known sim_num or None)."""
    nums = []
    for name, t in (("max_similarity", max_similarity), ("max_known_similarity", max_known_similarity)):
        if t is None:
            nums.append(None)
            continue
        if isinstance(t, bool) or not isinstance(t, (int, float)) or not 0 < t <= 1:
            raise ValueError(f"{name} must be a float in (0, 1], got {t!r}")
        num = int(round(t * FP_SIM_DEN))
        if not 1 <= num <= FP_SIM_DEN:
            raise ValueError(f"{name} = {t!r} is sim_num = {num} of {FP_SIM_DEN}, outside [1, {FP_SIM_DEN}]")
        nums.append(num)
    if nums == [None, None]:
        return None, None
    _radius_arg(fingerprint_radius)
    if vocabulary is None:
        raise ValueError("max_similarity / max_known_similarity read the rows as strings: give a vocabulary")
    if length > MAX_MOL_LENGTH:
        raise ValueError(f"tokens has rows of {length} positions; the fingerprint takes at most {MAX_MOL_LENGTH} "
                         "(wider rows are out of scope)")
    if nums[1] is not None and (known is None or len(known) == 0):
        raise ValueError(f"max_known_similarity = {max_known_similarity} asks for the similarity to the known set: give a non-empty "
                         "known_tokens")
    return nums[0], nums[1]


def _screen(model_forward, tokens, conditioning, device, candidates, keep, *, known_tokens=None, weights=None,
            forward_timesteps=100, X_norm_factor=1.0, forward_noise=None, sampler=None, sigma_schedule=None, min_distance=1,
            min_novelty=1, vocabulary=None, identity="string", max_similarity=None, max_known_similarity=None,
            fingerprint_radius=2, require=None, forbid=None, kekulize=False, limits=None, max_per_scaffold=None,
            novel_scaffold=False, scaffold_exocyclic=True, scaffold_generic=False, normalize=False, counts=None) -> Screened:
    """screen_tokens and screen_tokens_diverse; with both filters at 1 this is screen_tokens' sequence, launch for launch.  With a
    ``vocabulary`` one mdt::smiles_check over the N * G rows goes in front of the selection, which takes its status as `reject`;
    with ``identity="graph"`` mdt::mol_graph -> mdt::mol_key -> mdt::key_flags follow it and their bits 4 / 8 are OR-ed into `reject`;
    with ``require`` / ``forbid`` one mdt::sub_match on the same graph ORs bit 128 in, and with ``counts`` one mdt::sub_map after it does;
    with ``kekulize`` one mdt::mol_hydrogens on the
    same graph, right after mdt::mol_graph, ORs bit 64 in where its verdict is not 0; with ``limits`` one mdt::mol_rings after that
    mdt::mol_hydrogens (made once when both are asked for) ORs bit 128 in where a descriptor lies outside its bounds; with
    ``normalize`` one mdt::mol_normalize follows those two launches (made for it where nobody else asked) and mdt::mol_key,
    mdt::sub_match and mdt::mol_fp read its graph, the known set's keys and fingerprints being the normalised ones; with
    ``max_per_scaffold`` / ``novel_scaffold`` one mdt::mol_scaffold -> mdt::mol_key on that graph gives every row its scaffold key,
    which the selection (mdt::screen_select_classes) takes as `class_key` and mdt::key_flags looks up in the known set's."""
    weights, known = _screen_args(conditioning, candidates, keep, known_tokens, weights, tokens=tokens)
    diverse = _diverse_args(min_distance, min_novelty, known, tokens=tokens)
    width = torch.as_tensor(tokens).shape[1]
    _vocabulary_arg(vocabulary, width)
    _identity_arg(identity, vocabulary, width)
    sim_num, known_sim_num = _similarity_args(max_similarity, max_known_similarity, fingerprint_radius, vocabulary, known, width)
    fragments = _substructure_args(require, forbid, vocabulary, width)
    _kekulize_arg(kekulize, vocabulary, width)
    _limits_arg(limits, vocabulary, width)
    scaffold_mode = _scaffold_args(max_per_scaffold, novel_scaffold, scaffold_exocyclic, scaffold_generic, vocabulary, known, width)
    _counts_arg(counts, vocabulary, width)
    _screen_normalize_arg(normalize, vocabulary, width, identity == "graph" or sim_num is not None or known_sim_num is not None or
                          fragments is not None or scaffold_mode is not None or counts is not None)
    device = torch.device(device)
    N, K = candidates, keep
    G, n = conditioning.shape
    tok = torch.as_tensor(tokens).to(device)
    if n > model_forward.max_length:
        raise ValueError(f"conditioning holds {n} properties, the forward model predicts {model_forward.max_length} positions")
    packed, length, key, data = torch.ops.mdt.tokens_compact(tok, model_forward.max_length, float(X_norm_factor))
    result = model_forward.sample(data, device, cond_scale=1.0, timesteps=forward_timesteps, clamp=False, noise=forward_noise,
                                  sampler=sampler, sigma_schedule=sigma_schedule)
    target = conditioning.detach().to(device=device, dtype=torch.float32)
    score = torch.ops.mdt.screen_score(result, target, None if weights is None else weights.to(device), N)
    kk, kp, kl = known.on(device) if known is not None and len(known) else (None, None, None)
    reject = None
    if vocabulary is not None:                                   # is it a molecule at all?  bits 32 / 64, never kept
        reject, _ = torch.ops.mdt.smiles_check(packed, length, *vocabulary.on(device))
    graph = None
    if kekulize or limits is not None or normalize:              # the hydrogens: one launch for the Kekule check, the descriptors
        graph = torch.ops.mdt.mol_graph(packed, length, *vocabulary.on(device))[:4]      # and the normal form
        hydrogens, partner, verdict, _, _ = torch.ops.mdt.mol_hydrogens(*graph, MOLH_MAX_STEPS)
    if kekulize:                                                 # can its aromatic atoms be satisfied?  bit 64, never kept
        reject = reject | ((verdict != 0).to(torch.uint8) * rt.SCREEN_OVERVALENT)
    if limits is not None or normalize:                          # the rings: one launch for the bounds and the normal form
        bounds = limits.on(device) if limits is not None else (None, None)
        bond_ring, _, _, outside = torch.ops.mdt.mol_rings(*graph, hydrogens, *bounds)
    if limits is not None:                                       # is it inside the descriptor bounds?  bit 128, never kept
        reject = reject | outside                                # (the graph as written)
    if normalize:                                                # from here on the graph is its normal form
        graph = _normal_form(*graph, hydrogens, partner, verdict, bond_ring)[0]
    if identity == "graph":                                      # which molecule is it?  bits 4 / 8 by the graph key
        if graph is None:
            graph = torch.ops.mdt.mol_graph(packed, length, *vocabulary.on(device))[:4]
        graph_key = torch.ops.mdt.mol_key(*graph)
        known_graph = known.mol_keys(vocabulary, device, normalize=normalize) if known is not None and len(known) else None
        reject = reject | torch.ops.mdt.key_flags(graph_key, N, known_graph)
    if fragments is not None:                                    # does it contain the fragment?  bit 128, never kept
        if graph is None:
            graph = torch.ops.mdt.mol_graph(packed, length, *vocabulary.on(device))[:4]
        reject = reject | torch.ops.mdt.sub_match(*graph, *_joined_patterns(fragments[0], device), fragments[1], fragments[2])[2]
    if counts is not None:                                       # how often does it contain the fragment?  bit 128, never kept
        if graph is None:
            graph = torch.ops.mdt.mol_graph(packed, length, *vocabulary.on(device))[:4]
        reject = reject | torch.ops.mdt.sub_map(*graph, *counts.set.on(device), *counts.on(device))[5]
    fp = fp_count = None
    if sim_num is not None or known_sim_num is not None:         # how similar is it?  fingerprints of the graph, computed once
        if graph is None:
            graph = torch.ops.mdt.mol_graph(packed, length, *vocabulary.on(device))[:4]
        fp, fp_count = torch.ops.mdt.mol_fp(*graph, fingerprint_radius)
    if known_sim_num is not None:                                # bit 8 where the nearest known molecule is at least that similar
        known_fp, _ = known.fingerprints(vocabulary, device, fingerprint_radius, normalize=normalize)
        _, inter, union = torch.ops.mdt.fp_nearest(fp, known_fp)
        near = (union > 0) & (inter.long() * FP_SIM_DEN >= known_sim_num * union.long())     # the integer rule of mdt_hip.h
        reject = reject | (near.to(torch.uint8) * rt.SCREEN_KNOWN)
    class_key = None
    if scaffold_mode is not None:                                # which ring framework is it built on?  the key of its scaffold
        if graph is None:
            graph = torch.ops.mdt.mol_graph(packed, length, *vocabulary.on(device))[:4]
        ring_key = torch.ops.mdt.mol_key(*torch.ops.mdt.mol_scaffold(*graph, scaffold_mode)[:4])
        if novel_scaffold:                                       # bit 8 where the known set holds that scaffold (key 0: never)
            known_rings = known.scaffold_keys(vocabulary, device, normalize=normalize, exocyclic=scaffold_exocyclic,
                                              generic=scaffold_generic)
            reject = reject | (torch.ops.mdt.key_flags(ring_key, N, known_rings) & rt.SCREEN_KNOWN)
        if max_per_scaffold is not None:                         # at most that many kept per scaffold: the selection's classes
            class_key = ring_key
    distances = diverse or sim_num is not None or class_key is not None     # the selections that take known_dist and the two minima
    known_dist = None
    if distances and min_novelty > 1:                            # novelty as a distance: the nearest known row of every candidate
        known_dist, _ = torch.ops.mdt.edit_nearest(packed, length, kp, kl)
        kk = kp = kl = None
    args = (score, key, packed, length, N, K, kk, kp, kl)
    if distances:
        args += (known_dist, min_novelty, min_distance)
    if class_key is not None:
        if sim_num is None:                                      # (fingerprints made for the known set alone are not the selection's)
            fp = fp_count = None
        status, index, count = torch.ops.mdt.screen_select_classes(*args, reject, fp, fp_count, sim_num or 0, class_key,
                                                                   max_per_scaffold)
    elif sim_num is not None:
        status, index, count = torch.ops.mdt.screen_select_similar(*args, reject, fp, fp_count, sim_num)
    elif reject is not None:
        select = torch.ops.mdt.screen_select_diverse_reject if diverse else torch.ops.mdt.screen_select_reject
        status, index, count = select(*args, reject)
    else:
        select = torch.ops.mdt.screen_select_diverse if diverse else torch.ops.mdt.screen_select
        status, index, count = select(*args)
    index = index.long()
    filled = index >= 0
    rows = index.clamp(min=0) * G + torch.arange(G, device=device).unsqueeze(1)
    props = result.reshape(N * G, -1)[:, :n]
    return Screened(tokens=torch.where(filled.unsqueeze(2), tok.long()[rows], 0),
                    props=torch.where(filled.unsqueeze(2), props[rows], float("nan")),
                    score=torch.where(filled, score[rows], float("inf")),
                    index=index, count=count.long(), status=status.view(N, G))


def screen_tokens(model_forward: "QMDiffusionForward", tokens: Tensor, conditioning: Tensor, device, candidates: int, keep: int, *,
                  known_tokens=None, weights=None, forward_timesteps: int = 100, X_norm_factor: float = 1.0, forward_noise=None,
                  sampler=None, sigma_schedule=None) -> Screened:
    """The last mile of the reference's callers (sample_loop_generative / generate_from_conditioning, generative.py:1196-1291,
    :1685-1738) for N = ``candidates`` tries per target: re-predict the properties of the generated molecules with the forward
    model, compare them with the target, drop what is empty, repeated or already known (is_novel, :1063), keep the K = ``keep``
    best per target -- without leaving the device.

    ``tokens``: (N * G, L) ids from ANY producer (sample_tokens, inpaint_tokens, refine_tokens), row c * G + g = candidate c of
    target g -- the layout of guidance_sweep and of ``conditioning.repeat(N, 1)``; ``conditioning``: (G, n), the targets.
    A molecule is its compacted id row -- the non-zero ids in order, which is the reference's string: its tokenizer is
    character-level and skips id 0 -- so two rows that differ only in where their zeros sit are the same molecule.
    ``known_tokens``: a KnownSet, or raw (M, L_any) ids (wrapped; build the KnownSet once when calling repeatedly).
    ``weights``: (n,) non-negative; score = sum_i w_i (p_i - t_i)^2 / n on the scaled properties (None: all 1).
    Sequence: mdt::tokens_compact -> model_forward.sample on the compacted input (tokens_to_forward_input's, bit for bit) ->
    mdt::screen_score -> mdt::screen_select -> a gather.  Of equal molecules in a group the lowest c stands for all; ties in the
    score go to the lower c.  Returns Screened; the reference's "fraction of novel structures" is
    ``((status & 8) == 0).float().mean()``."""
    return _screen(model_forward, tokens, conditioning, device, candidates, keep, known_tokens=known_tokens, weights=weights,
                   forward_timesteps=forward_timesteps, X_norm_factor=X_norm_factor, forward_noise=forward_noise, sampler=sampler,
                   sigma_schedule=sigma_schedule)


def screen_tokens_diverse(model_forward: "QMDiffusionForward", tokens: Tensor, conditioning: Tensor, device, candidates: int,
                          keep: int, *, min_distance: int = 1, min_novelty: int = 1, vocabulary=None, identity: str = "string",
                          max_similarity=None, max_known_similarity=None, fingerprint_radius: int = 2, require=None, forbid=None,
                          kekulize: bool = False, limits=None, max_per_scaffold: Optional[int] = None, novel_scaffold: bool = False,
                          scaffold_exocyclic: bool = True, scaffold_generic: bool = False, counts=None, normalize: bool = False,
                          **screen_tokens_kwargs) -> Screened:
    """screen_tokens (whose keyword arguments this takes) with "distinct" and "novel" measured in edits: the Levenshtein distance
    (insert, delete, substitute: 1 each) between the compacted id rows, i.e. between the molecules' strings -- and, with
    ``vocabulary=``, with "is it a molecule at all?" asked of every candidate.

    ``vocabulary``: a SmilesVocabulary (None: not asked; the call makes the launches it made before, in the same order).  One
    mdt::smiles_check (see smiles_check() for what it does and does not check) runs over the N * G compacted rows and the selection
    takes its status as `reject`: a malformed candidate gets status bit 32 (runtime.SCREEN_MALFORMED), an overvalent one bit 64
    (runtime.SCREEN_OVERVALENT); neither is kept, and neither pushes another candidate out under ``min_distance``.  The valid
    fraction is ``((status & 96) == 0).float().mean()``.  It works with both filters at 1 as well (screen_tokens plus validity)
    and needs rows of at most 128 positions, refused with ValueError before anything is launched.

    ``min_distance``: the K kept molecules of a target lie at least this many edits apart.  The eligible candidates are taken in
    (score, c) order; one that is closer than ``min_distance`` to a candidate kept before it is passed over and gets status bit 16
    (runtime.SCREEN_CLOSE), so ``count`` may stay below K although eligible candidates are left.  1: distinct rows, as screen_tokens.
    ``min_novelty``: a candidate closer than this many edits to ANY molecule of ``known_tokens`` counts as known: status bit 8 then
    means "within min_novelty - 1 edits of the known set" (1: "in the known set", the hash lookup of screen_tokens), and the
    reference's "fraction of novel structures" stays ``((status & 8) == 0).float().mean()``.  Above 1 it needs a non-empty known
    set and runs mdt::edit_nearest once over all N * G rows.
    Both are ints >= 1; (1, 1) is screen_tokens itself, the same launches in the same order.  Either above 1 routes the selection to
    mdt::screen_select_diverse and needs rows of at most 64 positions and ids in [0, 64), in the tokens (one aminmax: the one host
    synchronisation added) and in the known set (checked once per KnownSet) -- all refused with ValueError before anything is
    launched.  Rows of more than one 64-bit word are out of scope.

    ``identity``: what "the same molecule" means for status bits 4 (duplicate) and 8 (known).  ``"string"`` (the default): equality
    of the compacted id rows, exactly the launches made without the keyword, in the same order.  ``"graph"``: equality of the graph
    key of mol_key() as well, so OCC after CCO is a duplicate, and known when the known set spells it C(O)C -- see mol_key() for
    what the key is and is not (a refinement hash, not a canonical form; no hydrogen, aromaticity or stereo normalisation).  It needs
    a ``vocabulary`` and rows of at most 64 positions, refused with ValueError before anything is launched.  After
    mdt::smiles_check it runs mdt::mol_graph -> mdt::mol_key -> mdt::key_flags (the known set's keys: KnownSet.mol_keys(), computed
    once) and ORs the flags into the `reject` byte of the selection.  Equal strings are equal graphs, so graph mode only adds bits;
    of the spellings of one molecule in a group the lowest c stands for all.  ``min_distance`` and ``min_novelty`` stay measured
    in edits on the STRINGS in both modes, and the novel fraction stays ``((status & 8) == 0).float().mean()``.

    ``max_similarity`` / ``max_known_similarity``: "distinct" and "novel" measured on the GRAPHS instead, as the Tanimoto similarity
    of the fingerprints of mol_fingerprint() (radius ``fingerprint_radius``, 0..3) -- see there for what the fingerprint is and is
    not: not RDKit's Morgan or ECFP, no implicit hydrogens, no aromaticity perception, no stereo, and folding can make unequal
    molecules look alike.  Each is None (off) or a float in (0, 1], handed to the kernels as ``sim_num = int(round(t * 65536))``
    and compared exactly (``inter * 65536 >= sim_num * union``); both need a ``vocabulary`` and rows of at most 64 positions.
    ``max_similarity``: a candidate at least that similar to a candidate kept before it is passed over and gets status bit 16; the
    selection is routed to mdt::screen_select_similar and combines with ``min_distance`` (either test passes a candidate over).
    ``max_known_similarity``: needs a non-empty known set; mdt::fp_nearest runs once over the N * G rows against
    KnownSet.fingerprints() and bit 8 is OR-ed into `reject` where the nearest known molecule is at least that similar.  A row that
    is no molecule has an all-zero fingerprint, similar to nothing.  With both at None nothing new is launched; refusals come
    with ValueError before anything is launched.

    ``require`` / ``forbid``: fragments a kept candidate must contain / may not contain, as GRAPHS (has_substructure(), see there
    for the definition and its limits: subgraph monomorphism on the graph of mol_graph() under a step cap; not SMARTS and not
    RDKit's HasSubstructMatch, no implicit hydrogens, no aromaticity perception, no stereo).  Each is a SubstructureSet, a list of
    SMILES strings (wrapped; build the set once when calling repeatedly) or None; together they hold at most 32 patterns; both need
    a ``vocabulary`` and rows of at most 64 positions.  One mdt::sub_match over the N * G rows -- on the graph that
    ``identity="graph"`` and the fingerprints use, computed once -- ORs status bit 128 (runtime.SCREEN_SUBSTRUCTURE) into `reject`
    where a required pattern is not found or a forbidden one is; an undecided verdict counts against the candidate both ways.  A
    candidate with bit 128 is never kept and pushes nothing out; ``((status & 128) == 0).float().mean()`` is the fraction that meets
    the constraint.  With both at None nothing new is launched.

    ``kekulize``: with True, "is it a molecule at all?" is also asked of the lower-case atoms, which mdt::smiles_check exempts from
    every valence rule (c1cccc1 passes it).  It needs a ``vocabulary`` and rows of at most 64 positions, refused with ValueError
    before anything is launched.  One mdt::mol_hydrogens (mol_hydrogens(), see there for the definition and its limits: not RDKit's
    sanitisation, ring membership is not checked, bracket atoms are taken at their word) runs over the N * G rows right after
    mdt::mol_graph -- the graph that ``identity="graph"``, the fingerprints and ``require`` / ``forbid`` share, computed once -- and
    rows whose verdict is not 0 get status bit 64 (runtime.SCREEN_OVERVALENT) OR-ed into `reject`.  No status bit is free, so under
    ``kekulize=True`` bit 64 also means "an aromatic atom's valence cannot be satisfied": an aromatic atom is overvalent, or no
    Kekule structure exists, or the search was undecided after 4096 steps, which counts against the row.  Such a row is never kept
    and pushes nothing out; the valid fraction stays ``((status & 96) == 0).float().mean()``.  With False (the default) the call
    makes exactly the launches it makes without the keyword, in the same order.

    ``limits``: a DescriptorLimits (None: not asked) -- bounds on the sixteen integer descriptors of mol_descriptors(): ring count
    and ring sizes, rotatable bonds, donors, acceptors, weight, ... (see there and mol_rings() for the definitions and their
    limits: not RDKit's ring info, not an SSSR, no logP, aromaticity as written).  It needs a ``vocabulary`` and rows of at most 64
    positions, refused with ValueError before anything is launched.  One mdt::mol_rings runs over the N * G rows after the shared
    mdt::mol_graph and after the mdt::mol_hydrogens launch that ``kekulize=True`` also uses -- that launch is made once when both
    are on -- and ORs status bit 128 (runtime.SCREEN_SUBSTRUCTURE) into `reject` where a descriptor of a molecule row lies outside
    its bounds.  No status bit is free, so under ``limits=`` bit 128 also means "a descriptor lies outside its bounds".  Such a
    candidate is never kept and pushes nothing out.  ``DescriptorLimits.lipinski()`` is weight <= 500, donors <= 5, acceptors <=
    10.  With None the call makes exactly the launches it makes without the keyword, in the same order.

    ``normalize``: True asks "which molecule is it?", "how similar?" and "does it contain the fragment?" of the NORMAL FORM of
    every row (mol_normalize(): hydrogens folded into the atoms, aromatic rings perceived by Hueckel's count on the Kekule
    structure), so that under ``identity="graph"`` OC1=CC=CC=C1 after c1ccccc1O gets bit 4 and a Kekule spelling of a known
    aromatic molecule bit 8, the similarity bounds compare fingerprints of normal forms, and ``forbid=["c1ccccc1"]`` rejects
    C1=CC=CC=C1 (aromatic fragments must then be written in lower case).  It needs a ``vocabulary``, rows of at most 64 positions
    and at least one consumer -- ``identity="graph"``, a similarity bound, or ``require`` / ``forbid`` -- refused with ValueError
    before anything is launched.  The launches: the one mdt::mol_graph, the one mdt::mol_hydrogens and the one mdt::mol_rings
    that ``kekulize`` / ``limits`` also use (never a second one), then one mdt::mol_normalize, after which mdt::mol_key /
    mdt::key_flags / mdt::sub_match / mdt::mol_fp read the normal form; the known set's keys and fingerprints are the normalised
    ones (KnownSet.mol_keys(normalize=True) / fingerprints(normalize=True), cached).  ``limits`` still reads the graph as
    written.  Its limits are mol_normalize()'s: not RDKit's aromaticity model, no envelope rings (azulene is not aromatic), no
    tautomers; a row whose Kekule verdict is not 0 is read as written.  With False (the default) the call makes exactly the
    launches it makes without the keyword, in the same order.

    ``max_per_scaffold`` / ``novel_scaffold``: "distinct" and "novel" asked of the RING FRAMEWORK a molecule is built on, the
    scaffold of mol_scaffold() (see there for the definition and its limits: the 2-core of the ring graph plus, with
    ``scaffold_exocyclic`` (default True), the atoms double-bonded to it; ``scaffold_generic`` (default False) compares frameworks
    with every atom a C and every bond single; not RDKit's MurckoScaffold, aromaticity and hydrogens as handed in, an acyclic
    molecule has NO scaffold).  Both need a ``vocabulary`` and rows of at most 64 positions, and both count as consumers of
    ``normalize``: with ``normalize=True`` the scaffold is read from the normal form, so a Kekule and an aromatic spelling share
    one.  One mdt::mol_scaffold -> mdt::mol_key runs over the N * G rows on the graph the call already has (mdt::mol_graph is never
    launched twice).  ``max_per_scaffold=m`` (an int >= 1, None: off): of the candidates of a target that share a scaffold key at most
    m are kept; one that finds m kept before it is passed over and gets status bit 16, as under ``min_distance``, with which and
    with ``max_similarity`` it combines (any test passes a candidate over); the selection goes to mdt::screen_select_classes.
    Candidates without a scaffold (key 0) are never counted.  ``novel_scaffold=True``: needs a non-empty known set; bit 8 is OR-ed
    into `reject` where the scaffold key is found in KnownSet.scaffold_keys() (computed once), so a new decoration of a known ring
    system counts as known.  Refusals come with ValueError before anything is launched.  With both at their defaults the call
    makes exactly the launches it makes without the keywords, in the same order.

    ``counts``: a SubstructureCounts (None: not asked) -- how OFTEN a kept candidate may contain fragments: "at most one nitro
    group", "at least two ring nitrogens".  What is counted is substructure_map()'s ``count`` (see there for the definition and
    its limits: anchors, not atom sets -- the atoms that can play the pattern's first atom; not SMARTS, a step cap, no stereo).
    It needs a ``vocabulary`` and rows of at most 64 positions, and counts as a consumer of ``normalize``.  One mdt::sub_map runs
    over the N * G rows on the graph the other filters read (after mdt::sub_match when ``require`` / ``forbid`` are given too) and
    ORs status bit 128 (runtime.SCREEN_SUBSTRUCTURE) into `reject` where a pattern's count lies outside its bounds; a start atom
    abandoned at the step cap counts against the candidate both ways.  Such a candidate is never kept and pushes nothing out.  With
    None the call makes exactly the launches it makes without the keyword, in the same order.
    Returns Screened, its six fields as screen_tokens'."""
    return _screen(model_forward, tokens, conditioning, device, candidates, keep, min_distance=min_distance, min_novelty=min_novelty,
                   vocabulary=vocabulary, identity=identity, max_similarity=max_similarity,
                   max_known_similarity=max_known_similarity, fingerprint_radius=fingerprint_radius, require=require, forbid=forbid,
                   kekulize=kekulize, limits=limits, max_per_scaffold=max_per_scaffold, novel_scaffold=novel_scaffold,
                   scaffold_exocyclic=scaffold_exocyclic, scaffold_generic=scaffold_generic, normalize=normalize, counts=counts,
                   **screen_tokens_kwargs)


# ----------------------------------------------------------------------------------------------------------------------
# is it a molecule at all?  well-formedness and valence of the strings behind the ids (csrc/k_smiles.hip)
# ----------------------------------------------------------------------------------------------------------------------
MAX_SMILES_LENGTH = 128         # mdt_smiles_check's limits (include/mdt_hip.h)
MAX_SMILES_ID = 256
VALENCE_SYMBOLS = ("B", "C", "N", "O", "P", "S", "F", "Cl", "Br", "I")
DEFAULT_MAX_VALENCE = dict(zip(VALENCE_SYMBOLS, (3, 4, 3, 2, 5, 6, 1, 1, 1, 1)))
ELEMENT_SYMBOLS = (
    "H He Li Be B C N O F Ne Na Mg Al Si P S Cl Ar K Ca Sc Ti V Cr Mn Fe Co Ni Cu Zn Ga Ge As Se Br Kr Rb Sr Y Zr Nb Mo Tc Ru Rh Pd "
    "Ag Cd In Sn Sb Te I Xe Cs Ba La Ce Pr Nd Pm Sm Eu Gd Tb Dy Ho Er Tm Yb Lu Hf Ta W Re Os Ir Pt Au Hg Tl Pb Bi Po At Rn Fr Ra "
    "Ac Th Pa U Np Pu Am Cm Bk Cf Es Fm Md No Lr Rf Db Sg Bh Hs Mt Ds Rg Cn Nh Fl Mc Lv Ts Og").split()
_SMILES_SYMBOLS = "-=#$:/\\().[]%@+*"           # classes 63 .. 78, in this order (include/mdt_hip.h, mdt_smiles_check)


def smiles_class(ch: str) -> int:
    """The class byte of one character (include/mdt_hip.h, mdt_smiles_check): 0 other | 1 + (c - 'A') | 27 + (c - 'a') |
    53 + digit | 63 + its place in ``- = # $ : / \\ ( ) . [ ] % @ + *``.  Only ASCII letters and digits count as such."""
    if len(ch) == 1 and ch.isascii():
        if ch.isupper():
            return 1 + ord(ch) - ord("A")
        if ch.islower():
            return 27 + ord(ch) - ord("a")
        if ch.isdigit():
            return 53 + int(ch)
        if ch in _SMILES_SYMBOLS:
            return 63 + _SMILES_SYMBOLS.index(ch)
    return 0


def element_masks():
    """The element table of mdt_smiles_check: numpy int32 (26,), bit k of word u set when (uppercase u, lowercase k) is one of the
    118 element symbols, bit 26 when the uppercase letter alone is."""
    import numpy as np
    masks = np.zeros(26, np.int64)
    for sym in ELEMENT_SYMBOLS:
        masks[ord(sym[0]) - ord("A")] |= 1 << (26 if len(sym) == 1 else ord(sym[1]) - ord("a"))
    return masks.astype(np.int32)


class SmilesVocabulary:
    """Which character each token id stands for -- what smiles_check() and the ``vocabulary=`` of the screening calls need to read
    an id row as a string.

    ``chars``: a sequence, ``chars[i]`` the character of id i (index 0 is ignored: id 0 is padding; ``None`` / ``""`` = unused),
    or a dict ``{id: char}`` such as a keras tokenizer's ``index_word``.  Characters are taken as given (no case folding).
    Entries of more than one character, ids outside [1, 256) and non-integer keys are refused with ValueError.
    ``max_valence``: overrides of the default maxima B 3, C 4, N 3, O 2, P 5, S 6, F 1, Cl 1, Br 1, I 1, e.g. ``{"N": 5}``; other
    keys, or values outside 0..8, are refused.
    ``classes`` uint8 (256), ``max_valence`` uint8 (10), ``elements`` int32 (26): numpy, the tables of mdt_smiles_check
    (include/mdt_hip.h).  ``class_id`` uint8 (128): the other way round for mol_write() -- the id that encodes each class of
    ``classes``, 0 where no character of the vocabulary has it; of two ids for one character the lower one encodes, as in encode().
    The device copies are made on first use and cached, one per device."""

    def __init__(self, chars, max_valence=None):
        import numpy as np
        if isinstance(chars, dict):
            items = list(chars.items())
        elif isinstance(chars, (str, bytes)) or not hasattr(chars, "__len__"):
            raise ValueError("chars must be a sequence of characters indexed by id, or a dict {id: character}")
        else:
            items = list(enumerate(chars))[1:]
        self.chars = {}
        for i, ch in items:
            if isinstance(i, (bool, float)) or not isinstance(i, (int, np.integer)):
                raise ValueError(f"token ids must be integers, got {i!r}")
            if ch is None or ch == "":
                continue
            if not isinstance(ch, str) or len(ch) != 1:
                raise ValueError(f"id {i} stands for {ch!r}: every id stands for exactly one character")
            if not 1 <= int(i) < MAX_SMILES_ID:
                raise ValueError(f"id {i} lies outside [1, {MAX_SMILES_ID})")
            self.chars[int(i)] = ch
        limits = dict(DEFAULT_MAX_VALENCE)
        for sym, v in (max_valence or {}).items():
            if sym not in limits:
                raise ValueError(f"max_valence: {sym!r} is none of {', '.join(VALENCE_SYMBOLS)}")
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v <= 8:
                raise ValueError(f"max_valence[{sym!r}] must be an int in 0..8, got {v!r}")
            limits[sym] = int(v)
        self.classes = np.zeros(MAX_SMILES_ID, np.uint8)
        for i, ch in self.chars.items():
            self.classes[i] = smiles_class(ch)
        self.max_valence = np.array([limits[sym] for sym in VALENCE_SYMBOLS], np.uint8)
        self.elements = element_masks()
        self._ids = {}
        for i in sorted(self.chars):
            self._ids.setdefault(self.chars[i], i)                         # (of two ids for one character the lower encodes)
        self.class_id = np.zeros(128, np.uint8)
        for i in sorted(self.chars, reverse=True):
            if self.classes[i]:
                self.class_id[self.classes[i]] = i
        self._on = {}
        self._class_id_on = {}

    def __len__(self) -> int:
        return len(self.chars)

    def encode(self, strings, length: int) -> Tensor:
        """-> int64 (R, length): one id per character, zero-padded at the end.  A character without an id, or a string of more
        than ``length`` characters, raises ValueError."""
        if isinstance(strings, str):
            strings = [strings]
        if isinstance(length, bool) or not isinstance(length, int) or length < 1:
            raise ValueError(f"length must be an int >= 1, got {length!r}")
        out = torch.zeros(len(strings), length, dtype=torch.int64)
        for r, s in enumerate(strings):
            if len(s) > length:
                raise ValueError(f"{s!r} has {len(s)} characters, the rows {length} positions")
            for j, ch in enumerate(s):
                if ch not in self._ids:
                    raise ValueError(f"{s!r}: the vocabulary has no id for {ch!r}")
                out[r, j] = self._ids[ch]
        return out

    def decode(self, ids):
        """-> list of str: the compacted rows (zeros anywhere are skipped) as strings.  An id without a character raises ValueError."""
        ids = _integer_ids(ids, "ids")
        rows = ids.detach().cpu().tolist() if isinstance(ids, Tensor) else ids.tolist()
        out = []
        for row in rows:
            try:
                out.append("".join(self.chars[t] for t in row if t != 0))
            except KeyError as e:
                raise ValueError(f"the vocabulary has no character for id {e.args[0]}") from None
        return out

    def on(self, device):
        """(classes uint8 (256), max_valence uint8 (10), elements int32 (26)) on ``device``."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._on:
            self._on[device] = tuple(torch.from_numpy(a).to(device) for a in (self.classes, self.max_valence, self.elements))
        return self._on[device]

    def class_id_on(self, device):
        """``class_id`` uint8 (128) on ``device``."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._class_id_on:
            self._class_id_on[device] = torch.from_numpy(self.class_id).to(device)
        return self._class_id_on[device]


def _vocabulary_arg(vocabulary, length: int) -> None:
    """The refusals of ``vocabulary=``, before anything is launched."""
    if vocabulary is None:
        return
    if not isinstance(vocabulary, SmilesVocabulary):
        raise ValueError(f"vocabulary must be a SmilesVocabulary, got {type(vocabulary).__name__}")
    if length > MAX_SMILES_LENGTH:
        raise ValueError(f"tokens has rows of {length} positions; smiles_check takes at most {MAX_SMILES_LENGTH} "
                         "(wider rows are out of scope)")


def smiles_check(tokens, vocabulary: "SmilesVocabulary", device):
    """Is each row a molecule at all?  -> (status int64 (R,), position int64 (R,)) for raw (R, L) ids of any integer dtype, zeros
    anywhere (a molecule is its compacted id row, as in screen_tokens), read as strings through ``vocabulary``.

    status 0: passes; 32 (runtime.SCREEN_MALFORMED): the string breaks the grammar -- atoms, bracket atoms, bonds, ring closures,
    branches, dots -- or leaves a ring or a branch open, ``position`` = the index of the first offending token in the compacted
    row, or the row's length where only the end shows it; 64 (runtime.SCREEN_OVERVALENT): well-formed, but the bond orders at an
    unbracketed atom exceed its maximum (``vocabulary.max_valence``), ``position`` = the lowest such atom.  An OK row (an empty
    one included) has position -1.  The rule set is written out at mdt_smiles_check in include/mdt_hip.h.

    This is a single pass over the string, not RDKit's MolFromSmiles (which the reference's draw_and_save asks,
    generative.py:954-994).  Not checked: aromaticity and kekulisation, two bonds between the same pair of atoms, hydrogens,
    bracket-atom valence, stereo consistency.  So 0 means "passes this check", not "RDKit parses it"; the intent is that what this
    check rejects RDKit rejects too (two known departures: '.' inside a branch, and %(nnn)) -- an intent that is unverified: it
    was never run against RDKit.
    L <= 128 and ids below 256 (an id outside [0, 256), or one without a character, is malformed where it stands); non-integer
    ids, L < 1 and L > 128 are refused with ValueError before anything is launched.  Sequence: mdt::tokens_compact ->
    mdt::smiles_check."""
    tok = _integer_ids(tokens, "tokens")
    if not isinstance(vocabulary, SmilesVocabulary):
        raise ValueError(f"vocabulary must be a SmilesVocabulary, got {type(vocabulary).__name__}")
    if tok.shape[1] < 1:
        raise ValueError("tokens must hold at least one position per row")
    _vocabulary_arg(vocabulary, tok.shape[1])
    device = torch.device(device)
    packed, n, _, _ = torch.ops.mdt.tokens_compact(torch.as_tensor(tok).to(device), 0, 1.0)
    status, position = torch.ops.mdt.smiles_check(packed, n, *vocabulary.on(device))
    return status.long(), position.long()


# ----------------------------------------------------------------------------------------------------------------------
# which molecule is it?  the graph behind a row and its spelling-invariant key (csrc/k_molgraph.hip): at most 64 positions
# ----------------------------------------------------------------------------------------------------------------------
def _identity_arg(identity, vocabulary, length: int) -> None:
    """The refusals of ``identity=``, before anything is launched."""
    if identity not in IDENTITIES:
        raise ValueError(f"identity must be one of {IDENTITIES}, got {identity!r}")
    if identity == "graph":
        if vocabulary is None:
            raise ValueError('identity="graph" reads the rows as strings: give a vocabulary')
        if length > MAX_MOL_LENGTH:
            raise ValueError(f"tokens has rows of {length} positions; the graph key takes at most {MAX_MOL_LENGTH} "
                             "(wider rows are out of scope)")


def _mol_rows(tokens, vocabulary, device):
    """The refusals of mol_graph() / mol_key(), then the compacted rows on the device."""
    tok = _integer_ids(tokens, "tokens")
    if not isinstance(vocabulary, SmilesVocabulary):
        raise ValueError(f"vocabulary must be a SmilesVocabulary, got {type(vocabulary).__name__}")
    if tok.shape[1] < 1:
        raise ValueError("tokens must hold at least one position per row")
    if tok.shape[1] > MAX_MOL_LENGTH:
        raise ValueError(f"tokens has rows of {tok.shape[1]} positions; the graph key takes at most {MAX_MOL_LENGTH} "
                         "(wider rows are out of scope)")
    packed, n, _, _ = torch.ops.mdt.tokens_compact(torch.as_tensor(tok).to(torch.device(device)), 0, 1.0)
    return packed, n


def mol_graph(tokens, vocabulary: "SmilesVocabulary", device):
    """The molecular graph behind each row -> (natoms int64 (R,), atoms int64 (R, L), nbonds int64 (R,), bonds int64 (R, L),
    status int64 (R,), position int64 (R,)) for raw (R, L) ids of any integer dtype, zeros anywhere, read through ``vocabulary``.

    ``status`` / ``position`` are smiles_check()'s.  For a row of status 0: ``atoms[r, :natoms[r]]`` are the atoms in order of
    appearance, one 32-bit descriptor each -- bits 0..4 the symbol's first letter (0..25; 26 for ``*``), 5..9 its second letter + 1
    (0: none), 10 aromatic (lower case), 11 bracket atom, 12..16 formal charge + 9, 17..20 bracket H count, 21..31 isotope modulo
    2048; chirality and atom class are ignored -- and ``bonds[r, :nbonds[r]]`` the bonds in order of creation,
    ``a | b << 8 | order << 16`` with ``- / \\`` 1, ``=`` 2, ``#`` 3, ``$`` 4, ``:`` 5, no symbol 5 between two aromatic atoms and
    1 otherwise.  A row of status != 0 and an empty row have no atoms; words beyond the counts are 0.  Atom and bond counts are what
    one filters on next.  The definition is written out at mdt_mol_graph in include/mdt_hip.h; it sees what smiles_check() sees and
    nothing more: no hydrogens beyond the bracket count, no aromaticity perception, no stereo.
    L <= 64 (64 tokens: at most 64 atoms, 63 bonds); the refusals are smiles_check()'s and L > 64, with ValueError before anything
    is launched.  Sequence: mdt::tokens_compact -> mdt::mol_graph."""
    packed, n = _mol_rows(tokens, vocabulary, device)
    out = torch.ops.mdt.mol_graph(packed, n, *vocabulary.on(torch.device(device)))
    natoms, atoms, nbonds, bonds, status, position = out
    return natoms.long(), atoms.long() & 0xFFFFFFFF, nbonds.long(), bonds.long(), status.long(), position.long()


def _normalize_arg(normalize) -> None:
    if not isinstance(normalize, bool):
        raise ValueError(f"normalize must be True or False, got {normalize!r}")


def _normal_form(natoms, atoms, nbonds, bonds, hydrogens=None, partner=None, verdict=None, bond_ring=None):
    """The normal form of graph arrays -> ((natoms, atoms', nbonds, bonds'), flags, verdict): mdt::mol_hydrogens -> mdt::mol_rings ->
    mdt::mol_normalize, the first two only where the caller has not made them already."""
    if hydrogens is None:
        hydrogens, partner, verdict, _, _ = torch.ops.mdt.mol_hydrogens(natoms, atoms, nbonds, bonds, MOLH_MAX_STEPS)
    if bond_ring is None:
        bond_ring = torch.ops.mdt.mol_rings(natoms, atoms, nbonds, bonds, hydrogens, None, None)[0]
    out_atoms, out_bonds, flags = torch.ops.mdt.mol_normalize(natoms, atoms, nbonds, bonds, hydrogens, partner, verdict, bond_ring)
    return (natoms, out_atoms, nbonds, out_bonds), flags, verdict


def _graph_rows(packed, n, vocabulary, device, normalize=False):
    """mdt::mol_graph on compacted rows -> ((natoms, atoms, nbonds, bonds), status, position); with ``normalize`` the graph is its
    normal form (_normal_form), without it nothing more is launched."""
    *graph, status, position = torch.ops.mdt.mol_graph(packed, n, *vocabulary.on(torch.device(device)))
    if normalize:
        graph = _normal_form(*graph)[0]
    return tuple(graph), status, position


def mol_key(tokens, vocabulary: "SmilesVocabulary", device, *, normalize: bool = False):
    """Which molecule is each row?  -> (key int64 (R,): the uint64 bits, status int64 (R,), position int64 (R,)) for raw (R, L) ids
    of any integer dtype, zeros anywhere.  ``key`` is a 64-bit key of the molecular graph behind the row (mol_graph()) that does not
    depend on how the row spells it: start atom, branch order, ring numbers (``%nn`` included), which end of a ring closure carries
    the bond symbol, an explicit ``-``, the order of dotted components.  OCC and CCO have one key; so have C1CC1C and CC1CC1.
    KEY 0 MEANS "NO MOLECULE": an empty row, or a row whose ``status`` (smiles_check()'s, with its ``position``) is not 0.

    The key is a rooted refinement hash (mdt_mol_key in include/mdt_hip.h has every step): for each atom as root, n rounds of
    neighbourhood hashing from the atom descriptors, all combinations sums mod 2^64.  Its limits:
    equal graphs always give equal keys; unequal graphs can collide in principle -- the key is a refinement hash, not a canonical
    form (none was found among 2,100 random graphs and the 684 small graphs it was tried on, and the rooting separates cubane from
    cuneane); and it is not RDKit's canonical SMILES, which the reference's callers would get (Chem.MolFromSmiles,
    generative.py:954-994).  These count as different molecules: [CH4] and C (no hydrogen or bracket normalisation);
    C1=CC=CC=C1 and c1ccccc1 (no aromaticity perception).  Stereo is ignored: F/C=C/F equals F/C=C\\F.
    ``normalize=True`` keys the normal form of mol_normalize() instead: there [CH4] and C, C1=CC=CC=C1 and c1ccccc1, and the two
    Kekule structures of one ring have one key (its limits are written at mol_normalize(): not RDKit's aromaticity model, no
    envelope rings, no tautomers); a row whose mol_hydrogens() verdict is not 0 is keyed as written.
    L <= 64; the refusals are smiles_check()'s and L > 64, with ValueError before anything is launched.
    Sequence: mdt::tokens_compact -> mdt::mol_graph -> mdt::mol_key; with ``normalize=True`` mdt::mol_hydrogens -> mdt::mol_rings ->
    mdt::mol_normalize go between the last two, with False exactly the launches named."""
    _normalize_arg(normalize)
    packed, n = _mol_rows(tokens, vocabulary, device)
    graph, status, position = _graph_rows(packed, n, vocabulary, device, normalize)
    key = torch.ops.mdt.mol_key(*graph)
    return key, status.long(), position.long()


# ----------------------------------------------------------------------------------------------------------------------
# how similar are two molecules?  Tanimoto similarity of graph fingerprints (csrc/k_molfp.hip): rows of at most 64 positions
# ----------------------------------------------------------------------------------------------------------------------
def _fp_of(tokens, vocabulary, device, radius, normalize=False):
    packed, n = _mol_rows(tokens, vocabulary, device)
    graph, status, position = _graph_rows(packed, n, vocabulary, device, normalize)
    fp, count = torch.ops.mdt.mol_fp(*graph, radius)
    return fp, count, status, position


def mol_fingerprint(tokens, vocabulary: "SmilesVocabulary", device, radius: int = 2, *, normalize: bool = False):
    """A circular fingerprint of the molecule behind each row -> (fp int64 (R, 16): the uint64 bits of 1024 bits, count int64 (R,):
    the set bits, status int64 (R,), position int64 (R,)) for raw (R, L) ids of any integer dtype, zeros anywhere.  ``status`` /
    ``position`` are smiles_check()'s.  A row that is no molecule (empty, or status != 0) has an all-zero fingerprint and count 0.

    On the graph of mol_graph(): every atom starts from its descriptor and its degree, and in each of ``radius`` rounds (0..3) takes
    in the labels of its neighbours with the bond orders -- the neighbourhood hash of mol_key() without a root; every atom sets one
    bit (label mod 1024) per round 0..radius.  mdt_mol_fp in include/mdt_hip.h has every step.  Equal graphs always give equal
    fingerprints, whatever the spelling: OCC and CCO have one fingerprint.  What it is NOT: it is not RDKit's Morgan or ECFP
    fingerprint, and its bits compare with neither; the round-0 invariant holds no implicit hydrogens; duplicate substructures are not
    removed; there is no aromaticity perception (C1=CC=CC=C1 and c1ccccc1 differ) and no stereo; and folding to 1024 bits can make
    unequal environments share a bit, so unequal molecules can reach similarity 1.  ``normalize=True`` fingerprints the normal form
    of mol_normalize() instead, in which hydrogens are folded into the atoms and aromatic rings are perceived (within its limits).
    L <= 64; the refusals are mol_key()'s and a radius outside [0, 3], with ValueError before anything is launched.
    Sequence: mdt::tokens_compact -> mdt::mol_graph -> mdt::mol_fp; with ``normalize=True`` mdt::mol_hydrogens -> mdt::mol_rings ->
    mdt::mol_normalize go between the last two."""
    radius = _radius_arg(radius)
    _normalize_arg(normalize)
    fp, count, status, position = _fp_of(tokens, vocabulary, device, radius, normalize)
    return fp, count.long(), status.long(), position.long()


def tanimoto(a_tokens, b_tokens, vocabulary: "SmilesVocabulary", device, radius: int = 2, *, normalize: bool = False):
    """How similar are the molecules of ``a_tokens`` and ``b_tokens``, row by row?  -> (similarity float32 (R,), inter int64 (R,),
    union int64 (R,)): the Tanimoto similarity of their mol_fingerprint()s, ``inter = popcount(A & B)``, ``union = |A| + |B| -
    inter``, ``similarity = inter / max(union, 1)`` computed in torch from the exact counts (compare the counts, not the floats,
    where exactness matters).  1 for two spellings of one molecule; 0 when either row is no molecule.  It is not RDKit's Morgan or
    ECFP similarity: no implicit hydrogens, no aromaticity perception, no stereo, duplicate substructures are not removed, and
    folding can make unequal molecules share bits (see mol_fingerprint()).  Both are raw (R, L) ids of the same shape, L <= 64.
    ``normalize=True`` compares the normal forms of mol_normalize(): c1ccccc1 and C1=CC=CC=C1 then have similarity 1.
    Sequence: per side mdt::tokens_compact -> mdt::mol_graph -> mdt::mol_fp, then mdt::fp_tanimoto."""
    radius = _radius_arg(radius)
    _normalize_arg(normalize)
    a, b = _integer_ids(a_tokens, "a_tokens"), _integer_ids(b_tokens, "b_tokens")
    if tuple(a.shape) != tuple(b.shape):
        raise ValueError(f"a_tokens {tuple(a.shape)} and b_tokens {tuple(b.shape)} must have the same shape")
    fa, fb = _fp_of(a, vocabulary, device, radius, normalize)[0], _fp_of(b, vocabulary, device, radius, normalize)[0]
    inter, union = torch.ops.mdt.fp_tanimoto(fa, fb)
    inter, union = inter.long(), union.long()
    return inter.float() / union.clamp(min=1).float(), inter, union


def nearest_known_tanimoto(tokens, known_tokens, vocabulary: "SmilesVocabulary", device, radius: int = 2, *,
                           normalize: bool = False):
    """Which known molecule is each molecule most similar to?  -> (similarity float32 (R,), index int64 (R,), inter int64 (R,),
    union int64 (R,)): the largest Tanimoto similarity (mol_fingerprint(), tanimoto()) of row r of ``tokens`` to any molecule of
    ``known_tokens`` -- a KnownSet, or raw ids, wrapped as screen_tokens does -- the LOWEST row of ``KnownSet.packed`` that attains
    it, and the exact counts of that pair (``similarity = inter / max(union, 1)``).  A row that is no molecule has similarity 0 and
    index 0.  The result does not depend on how the device splits the work.  It is not RDKit's Morgan or ECFP similarity (no
    implicit hydrogens, no aromaticity perception, no stereo; duplicate substructures are not removed; folding can make unequal
    molecules share bits).  L <= 64 in both; an empty known set has no nearest: refused with ValueError before anything is
    launched.  Sequence: mdt::tokens_compact -> mdt::mol_graph -> mdt::mol_fp -> mdt::fp_nearest (the known set's fingerprints:
    KnownSet.fingerprints(), computed once).  ``normalize=True`` compares normal forms (mol_normalize()) on both sides."""
    radius = _radius_arg(radius)
    _normalize_arg(normalize)
    tok = _integer_ids(tokens, "tokens")
    length = tok.shape[1]
    if not isinstance(vocabulary, SmilesVocabulary):
        raise ValueError(f"vocabulary must be a SmilesVocabulary, got {type(vocabulary).__name__}")
    if length < 1:
        raise ValueError("tokens must hold at least one position per row")
    if length > MAX_MOL_LENGTH:
        raise ValueError(f"tokens has rows of {length} positions; the fingerprint takes at most {MAX_MOL_LENGTH} "
                         "(wider rows are out of scope)")
    known = known_tokens if isinstance(known_tokens, KnownSet) else KnownSet(known_tokens, length)
    if known.width != length:
        raise ValueError(f"known_tokens was built for rows of {known.width} positions, tokens has {length}")
    if len(known) == 0:
        raise ValueError("known_tokens is empty: there is no nearest known molecule")
    fp = _fp_of(tok, vocabulary, device, radius, normalize)[0]
    known_fp, _ = known.fingerprints(vocabulary, device, radius, normalize=normalize)
    index, inter, union = torch.ops.mdt.fp_nearest(fp, known_fp)
    inter, union = inter.long(), union.long()
    return inter.float() / union.clamp(min=1).float(), index.long(), inter, union


# ----------------------------------------------------------------------------------------------------------------------
# does the molecule contain this fragment?  graph substructure match (csrc/k_molsub.hip): rows of at most 64 positions
# ----------------------------------------------------------------------------------------------------------------------
class SubstructureSet:
    """1 to 32 fragments to look for in molecules (has_substructure(), ``require=`` / ``forbid=`` of the screening calls): SMILES
    strings of at most 32 characters each, written in the dialect of smiles_check() and read through ``vocabulary`` -- not SMARTS.
    ``*`` accepts any atom; a bracket atom also wants its charge, H count and isotope; everything else wants its symbol and case.
    ``patterns`` (a tuple of str), ``vocabulary`` and ``len()`` are what it was built from.  An empty pattern, one of more than 32
    characters, a character without an id, no pattern or more than 32 raise ValueError here; a pattern that does not pass
    smiles_check() raises ValueError, naming the pattern and the position, on the first ``on(device)``."""

    def __init__(self, patterns, vocabulary: "SmilesVocabulary"):
        if not isinstance(vocabulary, SmilesVocabulary):
            raise ValueError(f"vocabulary must be a SmilesVocabulary, got {type(vocabulary).__name__}")
        if isinstance(patterns, str):
            patterns = [patterns]
        patterns = tuple(patterns)
        if not 1 <= len(patterns) <= MAX_SUB_PATTERNS:
            raise ValueError(f"a SubstructureSet holds 1 to {MAX_SUB_PATTERNS} patterns, got {len(patterns)}")
        for q, s in enumerate(patterns):
            if not isinstance(s, str):
                raise ValueError(f"pattern {q} is {s!r}: every pattern is a SMILES string")
            if s == "":
                raise ValueError(f"pattern {q} is empty at position 0: an empty fragment is in no molecule")
            if len(s) > MAX_SUB_LENGTH:
                raise ValueError(f"pattern {q} {s!r} has {len(s)} characters; a pattern takes at most {MAX_SUB_LENGTH} "
                                 "(wider patterns are out of scope)")
        self.patterns, self.vocabulary = patterns, vocabulary
        self.width = max(len(s) for s in patterns)
        self._tokens = vocabulary.encode(list(patterns), self.width)
        self._on = {}
        self._joined = {}

    def __len__(self) -> int:
        return len(self.patterns)

    def on(self, device):
        """The graphs of the patterns, (natoms int32 (P,), atoms int32 (P, LP), nbonds int32 (P,), bonds int32 (P, LP)) on
        ``device``: computed once per device by mdt::tokens_compact -> mdt::mol_graph and cached.  The first call per device
        costs one host synchronisation: a pattern that is malformed or overvalent raises ValueError with its position."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._on:
            packed, n, _, _ = torch.ops.mdt.tokens_compact(self._tokens.to(device), 0, 1.0)
            natoms, atoms, nbonds, bonds, status, position = torch.ops.mdt.mol_graph(packed, n, *self.vocabulary.on(device))
            status, position = status.cpu().tolist(), position.cpu().tolist()
            for q, (st, pos) in enumerate(zip(status, position)):
                if st != 0:
                    kind = "overvalent" if st == rt.SCREEN_OVERVALENT else "malformed"
                    raise ValueError(f"pattern {q} {self.patterns[q]!r} does not pass smiles_check(): {kind} at position {pos}")
            self._on[device] = (natoms, atoms, nbonds, bonds)
        return self._on[device]


def _substructure_set(patterns, vocabulary, what: str) -> "SubstructureSet":
    if isinstance(patterns, SubstructureSet):
        return patterns
    if isinstance(patterns, str) or not hasattr(patterns, "__len__"):
        raise ValueError(f"{what} must be a SubstructureSet or a list of SMILES strings, got {type(patterns).__name__}")
    return SubstructureSet(patterns, vocabulary)


def _substructure_args(require, forbid, vocabulary, length: int):
    """The refusals of ``require=`` / ``forbid=``, before anything is launched.  -> None when both are None, else (the sets in
    the order of their bits, need, ban)."""
    if require is None and forbid is None:
        return None
    if vocabulary is None:
        raise ValueError("require / forbid read the rows as strings: give a vocabulary")
    if not isinstance(vocabulary, SmilesVocabulary):
        raise ValueError(f"vocabulary must be a SmilesVocabulary, got {type(vocabulary).__name__}")
    if length > MAX_MOL_LENGTH:
        raise ValueError(f"tokens has rows of {length} positions; the substructure match takes at most {MAX_MOL_LENGTH} "
                         "(wider rows are out of scope)")
    sets, masks, at = [], [0, 0], 0
    for i, (what, given) in enumerate((("require", require), ("forbid", forbid))):
        if given is None:
            continue
        one = _substructure_set(given, vocabulary, what)
        sets.append(one)
        masks[i] = ((1 << len(one)) - 1) << at
        at += len(one)
    if at > MAX_SUB_PATTERNS:
        raise ValueError(f"require and forbid hold {at} patterns together; one call takes at most {MAX_SUB_PATTERNS}")
    return sets, masks[0], masks[1]


def _joined_patterns(sets, device):
    """The pattern graphs of one or two SubstructureSets as one set of arrays, the narrower padded with zeros; the joined arrays
    of a pair of sets are kept with the first of them, one per (second set, device)."""
    if len(sets) == 1:
        return sets[0].on(device)
    parts = [one.on(device) for one in sets]
    at = (id(sets[1]), parts[1][1].device)
    if at not in sets[0]._joined:
        width = max(p[1].shape[1] for p in parts)
        wide = lambda t: torch.nn.functional.pad(t, (0, width - t.shape[1]))  # noqa: E731
        joined = (torch.cat([p[0] for p in parts]), torch.cat([wide(p[1]) for p in parts]), torch.cat([p[2] for p in parts]),
                  torch.cat([wide(p[3]) for p in parts]))
        sets[0]._joined[at] = (sets[1], joined)                               # (the second set is held: its id stays its own)
    return sets[0]._joined[at][1]


def has_substructure(tokens, patterns, vocabulary: "SmilesVocabulary", device):
    """Does the molecule behind each row contain each fragment?  -> (match bool (R, P), undecided bool (R, P), status int64 (R,),
    position int64 (R,)) for raw (R, L) ids of any integer dtype, zeros anywhere, and ``patterns``, a SubstructureSet or a list
    of 1 to 32 SMILES strings of at most 32 characters (wrapped; build the set once when calling repeatedly).  ``status`` /
    ``position`` are smiles_check()'s; a row that is no molecule (empty, or status != 0) contains nothing, decided.

    On the graph of mol_graph(): pattern q occurs in a row when its atoms can be mapped to distinct atoms of the row so that every
    pattern atom accepts its image (equal symbol and case, ``*`` accepts all, a bracket atom also wants equal charge, H count and
    isotope) and every pattern bond finds a bond of the same order between the images -- subgraph monomorphism, so OCC contains CO,
    C1CC1 contains CCC, and a dotted pattern needs all its parts on distinct atoms.  mdt_sub_match in include/mdt_hip.h has every
    step, the order of the depth-first search included, because a root of the search that would take more than 4096 steps is
    abandoned: where no root succeeds and one was abandoned the pair is ``undecided`` (never together with ``match``).  A decided
    answer does not depend on how row or pattern is spelled; which pairs come out undecided can.  No pair was undecided among 54,000
    of small patterns and random molecules of up to 20 atoms; ``C.C.C.C.C.C.CN`` against 62 carbons and a lone N is.
    What it is NOT: not SMARTS and not RDKit's HasSubstructMatch.  There are no implicit hydrogens, so [CH4] does not accept C; no
    aromaticity perception, so c1ccccc1 is not found in C1=CC=CC=C1; no stereo, no recursive or logical atom expressions, and no
    mapping is returned (substructure_map() returns one, and counts).  (has_substructure_normalized() matches against the normal form of the rows, which lifts the first two.)
    The fingerprint of mol_fingerprint() is no pre-filter for this: an atom's degree enters its first
    round, so a fragment's bits are not a subset of its host's.
    L <= 64; non-integer ids, L < 1, L > 64, a vocabulary that is no SmilesVocabulary and patterns that SubstructureSet refuses
    raise ValueError before anything is launched.  Sequence: mdt::tokens_compact -> mdt::mol_graph -> mdt::sub_match (the
    patterns' graphs: SubstructureSet.on(), computed once)."""
    return _has_substructure(tokens, patterns, vocabulary, device, False)


def has_substructure_normalized(tokens, patterns, vocabulary: "SmilesVocabulary", device):
    """has_substructure() against the NORMAL FORM of the rows (mol_normalize()) -> the same four results.  The targets are
    normalised, the patterns are matched as written.  Every atom of a normalised target is a bracket atom with its hydrogens in
    its H field, so the bracket pattern [CH4] now accepts C, and [nH] accepts the N of C1=CNC=C1; aromaticity is perceived, so
    c1ccccc1 is found in C1=CC=CC=C1 and C1=CC=CC=C1 no longer is: AROMATIC FRAGMENTS MUST BE WRITTEN IN LOWER CASE, because the
    pattern's own case and bond orders are compared with the perceived ones.  A pattern atom without brackets accepts any hydrogen
    count, charge and isotope, as before; a bracket pattern atom wants the target's full hydrogen count ([CH3] does not accept the C
    of methane).  A row whose mol_hydrogens() verdict is not 0 is matched as written.  The limits are mol_normalize()'s (not RDKit's
    aromaticity model, no envelope rings) and has_substructure()'s (not SMARTS, a step cap, no stereo, no mapping).  The refusals
    are has_substructure()'s.  Sequence: mdt::tokens_compact -> mdt::mol_graph -> mdt::mol_hydrogens -> mdt::mol_rings ->
    mdt::mol_normalize -> mdt::sub_match."""
    return _has_substructure(tokens, patterns, vocabulary, device, True)


def _map_rows(tokens, patterns, vocabulary, normalize):
    """The refusals of has_substructure(), substructure_map() and substructure_keep(), before anything is launched -> (ids, the
    SubstructureSet)."""
    _normalize_arg(normalize)
    tok = _integer_ids(tokens, "tokens")
    if not isinstance(vocabulary, SmilesVocabulary):
        raise ValueError(f"vocabulary must be a SmilesVocabulary, got {type(vocabulary).__name__}")
    if tok.shape[1] < 1:
        raise ValueError("tokens must hold at least one position per row")
    if tok.shape[1] > MAX_MOL_LENGTH:
        raise ValueError(f"tokens has rows of {tok.shape[1]} positions; the substructure match takes at most {MAX_MOL_LENGTH} "
                         "(wider rows are out of scope)")
    return tok, _substructure_set(patterns, vocabulary, "patterns")


def _has_substructure(tokens, patterns, vocabulary, device, normalize):
    tok, fragments = _map_rows(tokens, patterns, vocabulary, normalize)
    packed, n = _mol_rows(tok, vocabulary, device)
    graph, status, position = _graph_rows(packed, n, vocabulary, device, normalize)
    match, undecided, _ = torch.ops.mdt.sub_match(*graph, *fragments.on(device), 0, 0)
    bit = torch.arange(len(fragments), device=match.device)
    spread = lambda word: ((word.long().unsqueeze(1) >> bit) & 1).bool()  # noqa: E731
    return spread(match), spread(undecided), status.long(), position.long()


# ----------------------------------------------------------------------------------------------------------------------
# which atoms match, and how often?  the enumeration behind the match (csrc/k_molsub.hip, k_sub_map)
# ----------------------------------------------------------------------------------------------------------------------
class SubstructureMap(NamedTuple):
    """What substructure_map() returns."""
    atom_map: Tensor      # (R, P, LP) int64: 1 + the row atom that pattern atom p maps to, 0 = none
    count: Tensor         # (R, P) int64: the anchors, popcount of ``found``
    found: Tensor         # (R, P, L) bool: the row atoms that can play pattern atom 0
    cover: Tensor         # (R, P, L) bool: the row atoms that lie in some embedding seen
    embeddings: Tensor    # (R, P) int64: the maps seen
    undecided: Tensor     # (R, P) bool: some root ran into the step cap
    status: Tensor        # (R,) int64, smiles_check()'s
    position: Tensor      # (R,) int64, smiles_check()'s


def _atom_bits(word, width: int):
    """(..., ) int64 words, the uint64 bits -> (..., width) bool, bit t at position t"""
    return ((word.unsqueeze(-1) >> torch.arange(width, device=word.device)) & 1).bool()


def substructure_map(tokens, patterns, vocabulary: "SmilesVocabulary", device, *, normalize: bool = False) -> SubstructureMap:
    """Which atoms of each row match each fragment, and how often?  -> SubstructureMap(atom_map int64 (R, P, LP), count int64 (R, P),
    found bool (R, P, L), cover bool (R, P, L), embeddings int64 (R, P), undecided bool (R, P), status int64 (R,), position int64
    (R,)) for raw (R, L) ids and ``patterns`` as has_substructure() takes them (LP: the widest pattern's characters).

    The definition is has_substructure()'s -- subgraph monomorphism on the graph of mol_graph(), pattern atoms in order of
    appearance, candidates in ascending atom index -- but every start atom (root) runs its depth-first search to the END instead of
    stopping at its first success; every full map met is an embedding.  mdt_sub_map in include/mdt_hip.h has every step.
    ``found[r, q, t]``: atom t of row r can play the FIRST atom of pattern q.  ``count`` is how many atoms can: it counts
    anchors, not atom sets.  C(F)(F)F counts CF3 carbons (each has 6 embeddings and is one anchor), [N+](=O)[O-] counts nitro
    nitrogens, and CC counts the carbons with a carbon neighbour, not the C-C bonds: WRITE THE FRAGMENT WITH ITS DISTINCTIVE ATOM
    FIRST.  ``embeddings`` is the number of maps seen (symmetric fragments are seen once per symmetry), ``cover`` the atoms in any of
    them.  ``atom_map[r, q, p]`` is 1 + the atom that pattern atom p maps to in the first map of the lowest found root (0: the
    pattern does not occur, or p is beyond its atoms), the lexicographically smallest embedding unless a lower root was capped.
    ``undecided[r, q]``: a root was abandoned after 4096 steps, so ``count`` may miss anchors, and ``embeddings`` / ``cover`` are
    lower bounds; where it is False all of them are exact and do not depend on how row or pattern is spelled (``atom_map`` names
    atoms in the row's own order of appearance, which does).  ``count > 0`` is has_substructure()'s ``match``; its ``undecided`` is
    ``count == 0`` and ``undecided`` here.  Enumeration runs into the cap more easily than the first-success search: a pattern of k
    equal dotted parts against n such atoms has n!/(n-k)! maps.
    ``normalize=True`` matches against the normal form of the rows (mol_normalize(), which keeps the atom numbering; the patterns
    are matched as written, see has_substructure_normalized()).
    What it is NOT: not SMARTS and not RDKit's GetSubstructMatches -- no implicit hydrogens, no aromaticity perception (without
    ``normalize``), no stereo, no uniquified atom sets.  A row that is no molecule has all-zero results.  The refusals are
    has_substructure()'s.  Sequence: mdt::tokens_compact -> mdt::mol_graph -> mdt::sub_map, with ``normalize=True``
    mdt::mol_hydrogens -> mdt::mol_rings -> mdt::mol_normalize after mdt::mol_graph."""
    tok, fragments = _map_rows(tokens, patterns, vocabulary, normalize)
    packed, n = _mol_rows(tok, vocabulary, device)
    graph, status, position = _graph_rows(packed, n, vocabulary, device, normalize)
    found, capped, embeddings, cover, atom_map, _ = torch.ops.mdt.sub_map(*graph, *fragments.on(device), None, None)
    found = _atom_bits(found, tok.shape[1])
    return SubstructureMap(atom_map.long(), found.sum(2), found, _atom_bits(cover, tok.shape[1]), embeddings.long(), capped != 0,
                           status.long(), position.long())


OCCURRENCES = ("all", "first")


def substructure_keep(tokens, patterns, vocabulary: "SmilesVocabulary", device, *, occurrences: str = "all", normalize: bool = False,
                      width=None, canonical: bool = False):
    """A lead respelled, and the mask of the tokens of its matched fragments -> (tokens int64 (R, width), keep_mask bool (R, width),
    matched bool (R, P), complete bool (R,), flags int64 (R,), status int64 (R,), position int64 (R,)): "keep this amide, vary
    the rest".  ``tokens`` is the lead respelled as scaffold_keep() does it (mol_write() with ``invariant=True``, ``width`` default
    the input's L, ``canonical`` as there); ``keep_mask`` is True exactly at the tokens that belong to an atom matched by ANY of
    the patterns -- the atom's text, its ring numbers, and the bond symbol and parentheses that lead to it -- and is the mask
    refine_keep_tokens(keep_mask=) takes.  ``occurrences="all"``: every atom in any embedding (substructure_map()'s ``cover``);
    ``"first"``: the atoms of the one returned map per pattern (``atom_map``, the first map of the lowest found root).
    ``matched[r, q]``: pattern q occurs in row r.  ``complete[r]`` is False where a root of that row ran into the step cap: atoms
    may be missing from the mask.  A row that was not written (``flags`` != 1, mol_write()'s) has an all-False mask.
    ``normalize=True``: the match reads the normal form (aromatic fragments in lower case, see has_substructure_normalized()), but
    the lead is written from the graph AS WRITTEN -- the model was trained on ordinary SMILES, and an all-bracket row is long and
    out of distribution; mol_normalize() keeps the atom numbering, so the matched atoms name the same tokens.
    The limits are substructure_map()'s (anchors, not atom sets; not SMARTS, a step cap, no stereo) and mol_write()'s (NOT RDKit's
    canonical SMILES).  The refusals are has_substructure()'s, ``occurrences`` outside ("all", "first"), ``width`` outside 1..128.
    Sequence: mdt::tokens_compact -> mdt::mol_graph -> mdt::sub_map -> mdt::mol_rank -> mdt::mol_canon (only with
    ``canonical=True``) -> mdt::mol_write, with ``normalize=True`` mdt::mol_hydrogens -> mdt::mol_rings -> mdt::mol_normalize
    after mdt::mol_graph; the mask is torch on the ops' outputs, no kernel of its own."""
    if occurrences not in OCCURRENCES:
        raise ValueError(f"occurrences must be one of {OCCURRENCES}, got {occurrences!r}")
    _canonical_arg(canonical, True)
    tok, fragments = _map_rows(tokens, patterns, vocabulary, normalize)
    width = _width_arg(width, tok.shape[1])
    packed, n = _mol_rows(tok, vocabulary, device)
    graph, status, position = _graph_rows(packed, n, vocabulary, device)
    found, capped, _, cover, atom_map, _ = torch.ops.mdt.sub_map(*(_normal_form(*graph)[0] if normalize else graph),
                                                                 *fragments.on(device), None, None)
    written, _, token_atom, flags = _write(graph, vocabulary, device, width, True, canonical)
    R, L = tok.shape
    if occurrences == "all":
        kept = torch.cat([torch.zeros(R, 1, dtype=torch.bool, device=cover.device), _atom_bits(cover, L).any(1)], dim=1)
    else:
        kept = torch.zeros(R, 1 + L, dtype=torch.bool, device=cover.device).scatter_(1, atom_map.long().view(R, -1), True)
        kept[:, 0] = False                                                   # (R, 1 + L): column 0 is "no atom"
    keep_mask = torch.gather(kept, 1, token_atom.long())
    return written.long(), keep_mask, found != 0, (capped == 0).all(1), flags.long(), status.long(), position.long()


class SubstructureCounts:
    """How often fragments may occur (``counts=`` of the screening calls): ``patterns`` as SubstructureSet takes them (or a
    SubstructureSet), with one lower bound ``at_least[q]`` and one upper bound ``at_most[q]`` per pattern, each an int >= 0 or None
    (no bound); ``at_least`` / ``at_most`` None: no such bound at all.  "At most one nitro group" is
    ``SubstructureCounts(["[N+](=O)[O-]"], v, at_most=[1])``, "at least two ring nitrogens" ``(["n"], v, at_least=[2])``.
    What is counted is substructure_map()'s ``count``: anchors, not atom sets -- the atoms that can play the pattern's FIRST atom,
    so write the fragment with its distinctive atom first; not SMARTS.  A start atom whose search was abandoned at the step cap
    counts against the row both ways.  ``set`` is the SubstructureSet, ``at_least`` / ``at_most`` tuples of ints (64 and more: no
    upper bound).  Bounds that are no ints >= 0, not one per pattern, or a lower bound above its upper one or above 64 raise
    ValueError here."""

    def __init__(self, patterns, vocabulary: "SmilesVocabulary", at_least=None, at_most=None):
        self.set = _substructure_set(patterns, vocabulary, "patterns")
        P = len(self.set)
        bounds = []
        for name, given, default in (("at_least", at_least, 0), ("at_most", at_most, 255)):
            given = [None] * P if given is None else given
            if isinstance(given, (str, int)) or not hasattr(given, "__len__") or len(given) != P:
                raise ValueError(f"{name} must be None or hold one bound per pattern ({P}), got {given!r}")
            for b in given:
                if b is not None and (isinstance(b, bool) or not isinstance(b, int) or b < 0):
                    raise ValueError(f"{name} holds {b!r}: every bound is an int >= 0 or None")
            bounds.append(tuple(default if b is None else min(b, 255) for b in given))
        self.at_least, self.at_most = bounds
        for q, (lo, hi) in enumerate(zip(*bounds)):
            if lo > hi or lo > MAX_MOL_LENGTH:
                raise ValueError(f"pattern {q} {self.set.patterns[q]!r}: no row has at least {lo} and at most {hi} of its "
                                 f"{MAX_MOL_LENGTH} atoms as anchors")
        self._on = {}

    def __len__(self) -> int:
        return len(self.set)

    def on(self, device):
        """(count_lo uint8 (P,), count_hi uint8 (P,)) on ``device``, made once per device"""
        device = torch.device(device)
        if device not in self._on:
            self._on[device] = tuple(torch.tensor(b, dtype=torch.uint8).to(device) for b in (self.at_least, self.at_most))
        return self._on[device]


def _counts_arg(counts, vocabulary, length: int) -> None:
    """The refusals of ``counts=``, before anything is launched."""
    if counts is None:
        return
    if not isinstance(counts, SubstructureCounts):
        raise ValueError(f"counts must be a SubstructureCounts or None, got {type(counts).__name__}")
    if vocabulary is None:
        raise ValueError("counts reads the rows as strings: give a vocabulary")
    if not isinstance(vocabulary, SmilesVocabulary):
        raise ValueError(f"vocabulary must be a SmilesVocabulary, got {type(vocabulary).__name__}")
    if length > MAX_MOL_LENGTH:
        raise ValueError(f"tokens has rows of {length} positions; the substructure match takes at most {MAX_MOL_LENGTH} "
                         "(wider rows are out of scope)")


# ----------------------------------------------------------------------------------------------------------------------
# how many hydrogens, and do the lower-case atoms add up?  implicit hydrogens, the Kekule check and the formula
# (csrc/k_molh.hip): rows of at most 64 positions
# ----------------------------------------------------------------------------------------------------------------------
FORMULA_SLOTS = ("H", "B", "C", "N", "O", "F", "P", "S", "Cl", "Br", "I", "other", "charge")      # the columns of mol_formula()
ATOMIC_WEIGHTS = dict(H=1.008, B=10.81, C=12.011, N=14.007, O=15.999, F=18.998403163, P=30.973761998, S=32.06, Cl=35.45, Br=79.904,
                      I=126.90447)                                # standard atomic weights (IUPAC abridged values)


def _kekulize_arg(kekulize, vocabulary, length: int) -> None:
    """The refusals of ``kekulize=``, before anything is launched."""
    if not isinstance(kekulize, bool):
        raise ValueError(f"kekulize must be True or False, got {kekulize!r}")
    if kekulize:
        if vocabulary is None:
            raise ValueError("kekulize=True reads the rows as strings: give a vocabulary")
        if length > MAX_MOL_LENGTH:
            raise ValueError(f"tokens has rows of {length} positions; the Kekule check takes at most {MAX_MOL_LENGTH} "
                             "(wider rows are out of scope)")


def _max_steps_arg(max_steps) -> int:
    if isinstance(max_steps, bool) or not isinstance(max_steps, int) or not 1 <= max_steps <= MOLH_MAX_STEPS:
        raise ValueError(f"max_steps must be an int in [1, {MOLH_MAX_STEPS}], got {max_steps!r}")
    return max_steps


def _hydrogens_of(tokens, vocabulary, device, max_steps):
    packed, n = _mol_rows(tokens, vocabulary, device)
    natoms, atoms, nbonds, bonds, status, position = torch.ops.mdt.mol_graph(packed, n, *vocabulary.on(torch.device(device)))
    return torch.ops.mdt.mol_hydrogens(natoms, atoms, nbonds, bonds, max_steps) + (status, position)


def mol_hydrogens(tokens, vocabulary: "SmilesVocabulary", device, max_steps: int = MOLH_MAX_STEPS):
    """How many hydrogens does each atom carry, and can the double bonds of the lower-case atoms be placed?  -> (hydrogens int64
    (R, L), partner int64 (R, L), verdict int64 (R,), atom int64 (R,), status int64 (R,), position int64 (R,)) for raw (R, L) ids of
    any integer dtype, zeros anywhere.  ``status`` / ``position`` are smiles_check()'s; the rest is indexed like mol_graph()'s atoms.

    ``hydrogens[r, a]``: the hydrogens of atom a -- a bracket atom's own count; for any other atom what fills its smallest normal
    valence (B 3, C 4, N 3 5, O 2, P 3 5, S 2 4 6, halogens 1) above its bonds, an aromatic bond counted as 1, less the one
    double bond an aromatic atom may still want.  ``verdict``: 0 the row adds up; 1 (runtime.MOLH_AROMATIC_OVERVALENT) an
    unbracketed aromatic atom has more bonds than any normal valence, ``atom`` = the lowest such atom (-1 otherwise); 2
    (runtime.MOLH_NO_KEKULE) the atoms that want a double bond cannot be paired along the aromatic bonds -- c1cccc1, n1cccc1
    (pyrrole without its H); 3 (runtime.MOLH_UNDECIDED) the pairing search made ``max_steps`` (1..4096) tries without an answer.
    ``partner[r, a]``: where the verdict is 0 and atom a wants a double bond, 1 + the atom it goes to, else 0 -- one Kekule
    structure; which one can depend on how the row is spelled, the verdict of a decided row, the hydrogens and the formula do not.
    A row that is no molecule (empty, or status != 0) has verdict 0, atom -1 and zeros.  mdt_mol_hydrogens in include/mdt_hip.h has
    every rule, the order of the search included, because its cap is part of the definition.
    What it is NOT: not RDKit's sanitisation.  Ring membership is not checked (cc is kekulisable as ethene), there is no
    aromaticity perception the other way (C1=CC=CC=C1 stays as written), no radicals, and bracket atoms are taken at their word.
    L <= 64; the refusals are mol_key()'s and a max_steps outside [1, 4096], with ValueError before anything is launched.
    Sequence: mdt::tokens_compact -> mdt::mol_graph -> mdt::mol_hydrogens."""
    max_steps = _max_steps_arg(max_steps)
    hydrogens, partner, verdict, atom, _, status, position = _hydrogens_of(tokens, vocabulary, device, max_steps)
    return hydrogens.long(), partner.long(), verdict.long(), atom.long(), status.long(), position.long()


def mol_formula(tokens, vocabulary: "SmilesVocabulary", device):
    """The molecular formula behind each row -> (counts int64 (R, 13), verdict int64 (R,), status int64 (R,), position int64 (R,))
    for raw (R, L) ids: the atoms of H B C N O F P S Cl Br I, of any other symbol (``*`` included), and the net formal charge
    (FORMULA_SLOTS), with the hydrogens of mol_hydrogens() -- see there for the rules and for ``verdict``, under which the counts are
    written whatever it is.  ``counts[:, 1:12].sum(1)`` is the heavy-atom count (a bracket atom [H] counts as a hydrogen); a row that
    is no molecule has all zeros.  formula_strings() and mol_weight() read the counts on the host.  Not RDKit's CalcMolFormula:
    no isotopes in the formula, no radicals.  L <= 64; the refusals are mol_key()'s.
    Sequence: mdt::tokens_compact -> mdt::mol_graph -> mdt::mol_hydrogens."""
    _, _, verdict, _, formula, status, position = _hydrogens_of(tokens, vocabulary, device, MOLH_MAX_STEPS)
    return formula.long(), verdict.long(), status.long(), position.long()


def _formula_counts(counts):
    counts = torch.as_tensor(counts).detach().cpu()
    if counts.dim() != 2 or counts.shape[1] != len(FORMULA_SLOTS) or counts.is_floating_point():
        raise ValueError(f"counts must be integers of shape (R, {len(FORMULA_SLOTS)}) as mol_formula() returns them, got "
                         f"{counts.dtype} {tuple(counts.shape)}")
    return counts.long()


def formula_strings(counts):
    """The rows of mol_formula()'s ``counts`` as text, on the host: Hill order (C, H, then the other symbols alphabetically; without
    carbon all alphabetically), a count of 1 not written, the net charge as ``+`` / ``-`` / ``+2`` / ``-2``, a ``?`` at the end when
    atoms of other symbols are present (they are not in the text), and ``""`` for a row without atoms.  C2H6O, H4N+, CH3?."""
    out = []
    for row in _formula_counts(counts).tolist():
        count = dict(zip(FORMULA_SLOTS, row))
        if not any(row[:12]):
            out.append("")
            continue
        symbols = sorted(FORMULA_SLOTS[:11])
        if count["C"]:
            symbols = ["C", "H"] + [s for s in symbols if s not in ("C", "H")]
        text = "".join(s + (str(count[s]) if count[s] != 1 else "") for s in symbols if count[s])
        q = count["charge"]
        if q:
            text += ("+" if q > 0 else "-") + (str(abs(q)) if abs(q) > 1 else "")
        out.append(text + ("?" if count["other"] else ""))
    return out


def mol_weight(counts) -> Tensor:
    """The molecular weight of the rows of mol_formula()'s ``counts``, on the host: float64 (R,), the standard atomic weights
    (ATOMIC_WEIGHTS) times the counts; NaN where atoms of other symbols are present, 0 for a row without atoms.  Isotopes and the
    charge do not enter."""
    counts = _formula_counts(counts)
    w = torch.tensor([ATOMIC_WEIGHTS[s] for s in FORMULA_SLOTS[:11]], dtype=torch.float64)
    weight = counts[:, :11].double() @ w
    return torch.where(counts[:, 11] > 0, torch.full_like(weight, float("nan")), weight)


# ----------------------------------------------------------------------------------------------------------------------
# which bonds and atoms lie in a ring, and is the molecule inside the bounds?  ring perception and descriptors
# (csrc/k_molring.hip): rows of at most 64 positions
# ----------------------------------------------------------------------------------------------------------------------
DESCRIPTOR_NAMES = ("heavy_atoms", "hetero_atoms", "donors", "acceptors", "rotatable_bonds", "rings", "ring_atoms", "ring_bonds",
                    "smallest_ring", "largest_ring", "aromatic_atoms", "aromatic_outside_ring", "sp3_carbons", "carbons", "components",
                    "weight")                                    # the columns of mol_descriptors() (enum mdt_molr_slot)
_INT32_MIN, _INT32_MAX = -2 ** 31, 2 ** 31 - 1


class DescriptorLimits:
    """Bounds on the descriptors of mol_descriptors() for ``limits=`` of the screening calls: ``DescriptorLimits(max_rings=4,
    min_smallest_ring=5, max_rotatable_bonds=10, max_weight=500.0)``.  Every name of DESCRIPTOR_NAMES takes a ``min_<name>`` and a
    ``max_<name>`` keyword; both ends are inclusive, an unset bound is no bound (int32 min in ``lo``, int32 max in ``hi``), any other
    keyword raises ValueError.  The counts are ints; ``min_weight`` / ``max_weight`` are in dalton (int or float) and are handed to
    the kernel in milli-dalton, ``int(round(1000 * x))``, compared with the integer weight of mdt_mol_rings.  ``lo`` / ``hi``: int32
    (16,) on the host; ``on(device)`` keeps one copy per device.  Note ``min_smallest_ring=5`` also rejects a molecule without rings
    (its smallest ring is 0): "no three- or four-membered ring, rings or not" is not one pair of bounds."""

    def __init__(self, **bounds):
        lo, hi = [_INT32_MIN] * len(DESCRIPTOR_NAMES), [_INT32_MAX] * len(DESCRIPTOR_NAMES)
        for key, value in bounds.items():
            side, _, name = key.partition("_")
            if side not in ("min", "max") or name not in DESCRIPTOR_NAMES:
                raise ValueError(f"DescriptorLimits got {key!r}; the bounds are min_<name> / max_<name> for <name> in {DESCRIPTOR_NAMES}")
            if name == "weight":
                if isinstance(value, bool) or not isinstance(value, (int, float)) or value != value or abs(value) > 2.0e6:
                    raise ValueError(f"{key} must be a number of dalton in [-2e6, 2e6], got {value!r}")
                value = int(round(1000 * value))
            elif isinstance(value, bool) or not isinstance(value, int) or not _INT32_MIN <= value <= _INT32_MAX:
                raise ValueError(f"{key} must be an int (a count) inside int32, got {value!r}")
            (lo if side == "min" else hi)[DESCRIPTOR_NAMES.index(name)] = value
        self.bounds = dict(bounds)
        self.lo, self.hi = torch.tensor(lo, dtype=torch.int32), torch.tensor(hi, dtype=torch.int32)
        self._on = {}

    @classmethod
    def lipinski(cls) -> "DescriptorLimits":
        """Three of Lipinski's four rules: weight <= 500 dalton, donors <= 5 (N or O with a hydrogen), acceptors <= 10 (N + O).
        The fourth rule, logP <= 5, is not built: there is no logP here."""
        return cls(max_weight=500.0, max_donors=5, max_acceptors=10)

    def on(self, device):
        """(lo, hi) on ``device``, copied there once."""
        device = torch.device(device)
        if device not in self._on:
            self._on[device] = (self.lo.to(device), self.hi.to(device))
        return self._on[device]

    def __repr__(self):
        return "DescriptorLimits(%s)" % ", ".join(f"{k}={v!r}" for k, v in self.bounds.items())


def _limits_arg(limits, vocabulary, length: int) -> None:
    """The refusals of ``limits=``, before anything is launched."""
    if limits is None:
        return
    if not isinstance(limits, DescriptorLimits):
        raise ValueError(f"limits must be a DescriptorLimits or None, got {type(limits).__name__}")
    if vocabulary is None:
        raise ValueError("limits= reads the rows as strings: give a vocabulary")
    if length > MAX_MOL_LENGTH:
        raise ValueError(f"tokens has rows of {length} positions; the descriptors take at most {MAX_MOL_LENGTH} "
                         "(wider rows are out of scope)")


def _screen_normalize_arg(normalize, vocabulary, length: int, consumed: bool) -> None:
    """The refusals of the screening calls' ``normalize=``, before anything is launched."""
    _normalize_arg(normalize)
    if not normalize:
        return
    if vocabulary is None:
        raise ValueError("normalize=True reads the rows as strings: give a vocabulary")
    if length > MAX_MOL_LENGTH:
        raise ValueError(f"tokens has rows of {length} positions; the normal form takes at most {MAX_MOL_LENGTH} "
                         "(wider rows are out of scope)")
    if not consumed:
        raise ValueError('normalize=True changes what identity="graph", max_similarity / max_known_similarity and require / forbid '
                         "read: ask for one of them")


def _rings_of(tokens, vocabulary, device):
    packed, n = _mol_rows(tokens, vocabulary, device)
    *graph, status, position = torch.ops.mdt.mol_graph(packed, n, *vocabulary.on(torch.device(device)))
    hydrogens, _, verdict, _, _ = torch.ops.mdt.mol_hydrogens(*graph, MOLH_MAX_STEPS)
    bond_ring, atom_ring, desc, _ = torch.ops.mdt.mol_rings(*graph, hydrogens, None, None)
    return atom_ring, bond_ring, desc, verdict, status, position


def mol_rings(tokens, vocabulary: "SmilesVocabulary", device):
    """Which atoms and bonds lie in a ring, and how small is it?  -> (atom_ring int64 (R, L), bond_ring int64 (R, L), descriptors
    int64 (R, 16), verdict int64 (R,), status int64 (R,), position int64 (R,)) for raw (R, L) ids of any integer dtype, zeros
    anywhere.  ``status`` / ``position`` are smiles_check()'s; ``verdict`` is mol_hydrogens()'s, because donors and weight rest on
    its hydrogens (they are defined for every verdict); atoms and bonds are indexed like mol_graph()'s.

    ``bond_ring[r, e]``: the size of the smallest cycle through bond e -- 1 + the shortest path between its ends that avoids it --
    or 0 where there is none (a bridge).  ``atom_ring[r, a]``: the smallest non-zero value over the bonds at atom a, 0 for an atom
    in no ring.  The fusion bond of naphthalene is 6, every bond of cubane 4.  ``descriptors``: the columns of DESCRIPTOR_NAMES, see
    mol_descriptors().  A row that is no molecule (empty, or status != 0) has all zeros.  mdt_mol_rings in include/mdt_hip.h has
    every rule.
    What it is NOT: not RDKit's ring info and not an SSSR (nobody lists rings; ``rings`` is the cycle rank), no envelope rings,
    aromaticity is as written, not perceived.  L <= 64; the refusals are mol_key()'s, with ValueError before anything is launched.
    Sequence: mdt::tokens_compact -> mdt::mol_graph -> mdt::mol_hydrogens -> mdt::mol_rings."""
    return tuple(t.long() for t in _rings_of(tokens, vocabulary, device))


def mol_descriptors(tokens, vocabulary: "SmilesVocabulary", device):
    """Sixteen integer descriptors per row -> (descriptors int64 (R, 16), verdict int64 (R,), status int64 (R,), position int64
    (R,)) for raw (R, L) ids; the columns are DESCRIPTOR_NAMES: heavy atoms (symbol not H), hetero atoms (heavy and not C, ``*``
    counts), donors (N or O with a hydrogen), acceptors (N or O: Lipinski's N + O count), rotatable bonds (single, not in a ring,
    both ends with at least two heavy neighbours and no triple bond; an aromatic-order bond is never rotatable, which misses the
    axis of a biphenyl written without ``-``), rings (edges - atoms + components), ring atoms, ring bonds, smallest ring, largest
    ring (the largest of the bonds' smallest cycles: naphthalene 6), aromatic atoms (as written), aromatic atoms outside any ring
    (the ``cc`` that mol_hydrogens() accepts as ethene), sp3 carbons (C, not aromatic, single bonds only), carbons, components, and
    the weight in milli-dalton (the integer masses of mdt_mol_rings; atoms of other symbols weigh 0).  ``verdict`` is
    mol_hydrogens()'s.  No logP; not RDKit's descriptors.  The result does not depend on how a molecule is spelled.  L <= 64; the
    refusals are mol_key()'s.  Sequence: mdt::tokens_compact -> mdt::mol_graph -> mdt::mol_hydrogens -> mdt::mol_rings."""
    _, _, desc, verdict, status, position = _rings_of(tokens, vocabulary, device)
    return desc.long(), verdict.long(), status.long(), position.long()


# ----------------------------------------------------------------------------------------------------------------------
# one graph for the Kekule, the aromatic and the bracket spelling of a molecule: the normal form (csrc/k_molnorm.hip): rows of at
# most 64 positions
# ----------------------------------------------------------------------------------------------------------------------
def mol_normalize(tokens, vocabulary: "SmilesVocabulary", device):
    """The normal form of the molecular graph behind each row -> (natoms int64 (R,), atoms int64 (R, L), nbonds int64 (R,), bonds
    int64 (R, L), flags int64 (R,), verdict int64 (R,), status int64 (R,), position int64 (R,)) for raw (R, L) ids of any integer
    dtype, zeros anywhere.  ``natoms`` / ``nbonds`` / ``status`` / ``position`` and the indices of atoms and bonds are mol_graph()'s,
    ``verdict`` is mol_hydrogens()'s; ``atoms`` and ``bonds`` have mol_graph()'s format and are what mol_key(normalize=True),
    mol_fingerprint(normalize=True) and has_substructure_normalized() read.

    In the normal form every atom is a bracket atom that carries its hydrogens in its H field (at most 15), so [CH4] and C are one
    molecule; aromaticity is perceived, not read: the Kekule structure of mol_hydrogens() replaces the aromatic bonds, every atom
    gives 0, 1 or 2 pi electrons or is ineligible, and a smallest ring whose atoms are all eligible and give 2 mod 4 electrons
    (Hueckel) is aromatic -- its atoms get the aromatic bit, its bonds order 5, everything else its Kekule order -- so c1ccccc1 and
    C1=CC=CC=C1, and the two Kekule structures of any ring, are one molecule.  mdt_mol_normalize in include/mdt_hip.h has every
    rule.  ``flags``: 1 the row is normalised, 2 it has an aromatic ring, 4 an aromatic bit or bond order differs from what was
    written.  A row whose ``verdict`` is not 0 has no Kekule structure to read and comes back as written with flags 0; a row that is
    no molecule (empty, or status != 0) is all zero.  The normal form does not depend on the spelling but for the numbering of atoms
    and bonds; normalising it again changes nothing.
    What it is NOT: not RDKit's aromaticity model.  Rings are judged one at a time, so there are no envelope rings: azulene is NOT
    aromatic here, and RDKit says it is.  A bond in three or more equally small cycles (cubane-like) may try numbering-dependent
    rings.  A lower-case atom outside every perceived ring keeps the Kekule structure that mol_hydrogens() found (cc becomes C=C).
    No tautomers, no charge normalisation, no stereo.
    L <= 64; the refusals are mol_key()'s, with ValueError before anything is launched.
    Sequence: mdt::tokens_compact -> mdt::mol_graph -> mdt::mol_hydrogens -> mdt::mol_rings -> mdt::mol_normalize."""
    packed, n = _mol_rows(tokens, vocabulary, device)
    *graph, status, position = torch.ops.mdt.mol_graph(packed, n, *vocabulary.on(torch.device(device)))
    (natoms, atoms, nbonds, bonds), flags, verdict = _normal_form(*graph)
    return (natoms.long(), atoms.long() & 0xFFFFFFFF, nbonds.long(), bonds.long(), flags.long(), verdict.long(), status.long(),
            position.long())


# ----------------------------------------------------------------------------------------------------------------------
# which ring framework is a molecule built on?  the scaffold of a graph row (csrc/k_molscaf.hip): rows of at most 64 positions
# ----------------------------------------------------------------------------------------------------------------------
def _scaffold_mode(exocyclic, generic) -> int:
    """The refusals of ``exocyclic=`` / ``generic=`` -> the mode of mdt::mol_scaffold."""
    for name, v in (("exocyclic", exocyclic), ("generic", generic)):
        if not isinstance(v, bool):
            raise ValueError(f"{name} must be True or False, got {v!r}")
    return (rt.MOLS_EXOCYCLIC if exocyclic else 0) | (rt.MOLS_GENERIC if generic else 0)


def _scaffold_args(max_per_scaffold, novel_scaffold, exocyclic, generic, vocabulary, known, length: int):
    """The refusals of the screening calls' scaffold keywords, before anything is launched.  -> the mode of mdt::mol_scaffold, or
    None when neither ``max_per_scaffold`` nor ``novel_scaffold`` asks for a scaffold."""
    if max_per_scaffold is not None and (isinstance(max_per_scaffold, bool) or not isinstance(max_per_scaffold, int) or
                                         max_per_scaffold < 1):
        raise ValueError(f"max_per_scaffold must be an int >= 1 or None, got {max_per_scaffold!r}")
    if not isinstance(novel_scaffold, bool):
        raise ValueError(f"novel_scaffold must be True or False, got {novel_scaffold!r}")
    try:
        mode = _scaffold_mode(exocyclic, generic)
    except ValueError as e:
        raise ValueError("scaffold_" + str(e)) from None
    if max_per_scaffold is None and not novel_scaffold:
        return None
    if vocabulary is None:
        raise ValueError("max_per_scaffold / novel_scaffold read the rows as strings: give a vocabulary")
    if length > MAX_MOL_LENGTH:
        raise ValueError(f"tokens has rows of {length} positions; the scaffold takes at most {MAX_MOL_LENGTH} "
                         "(wider rows are out of scope)")
    if novel_scaffold and (known is None or len(known) == 0):
        raise ValueError("novel_scaffold=True asks whether the known set holds the scaffold: give a non-empty known_tokens")
    return mode


def _scaffold_of(tokens, vocabulary, device, normalize, exocyclic, generic):
    _normalize_arg(normalize)
    mode = _scaffold_mode(exocyclic, generic)
    packed, n = _mol_rows(tokens, vocabulary, device)
    graph, status, position = _graph_rows(packed, n, vocabulary, device, normalize)
    return torch.ops.mdt.mol_scaffold(*graph, mode), status, position


def mol_scaffold(tokens, vocabulary: "SmilesVocabulary", device, *, normalize: bool = False, exocyclic: bool = True,
                 generic: bool = False):
    """Which ring framework is each molecule built on?  -> (natoms int64 (R,), atoms int64 (R, L), nbonds int64 (R,), bonds int64
    (R, L), atom_map int64 (R, L), flags int64 (R,), status int64 (R,), position int64 (R,)) for raw (R, L) ids of any integer dtype,
    zeros anywhere.  ``status`` / ``position`` are smiles_check()'s.  The first four are graph arrays in mol_graph()'s format that
    hold the SCAFFOLD alone, renumbered: ``atom_map[r, a]`` is 1 + the scaffold index of atom a of mol_graph(), 0 for an atom that
    was pruned.  ``flags``: 1 the row is a molecule, 2 it has a scaffold, 4 the scaffold is the whole molecule.

    The scaffold is the 2-core of the ring graph: in rounds every atom with at most one neighbour left is removed, until none is;
    what stays is the atoms on a cycle or on a path between two cycles -- Bemis and Murcko's rings plus linkers, over all dotted
    components.  ``exocyclic=True`` (the default) also keeps an atom double-bonded to a kept one (the O of a ring C=O), and nothing
    that hangs on it.  A kept BRACKET atom adds what it lost to its H count (an entry of order o weighs o; at most 15), so on the
    normal form the [c] of toluene becomes the [cH] of benzene; an unbracketed atom stays as written, its hydrogens being implicit.
    ``generic=True`` makes every kept atom a plain C and every kept bond single: frameworks compared as bare graphs.
    ``normalize=True`` reads the normal form of mol_normalize() instead of the row as written, so that Cc1ccccc1 and CC1=CC=CC=C1
    have one scaffold.  mdt_mol_scaffold in include/mdt_hip.h has every rule.
    What it is NOT: not RDKit's MurckoScaffold.  Aromaticity and hydrogens are as handed in.  With ``exocyclic=False`` a ring C(=O)
    loses its O and gains two H when bracketed; on a normal form that can leave an aromatic atom with an odd H count.  Stereo is
    ignored.  An acyclic molecule has NO scaffold: all zero, scaffold_key() 0.  Applying it again with the same keywords is the
    identity, except with exocyclic and generic both on: GENERIC rewrites the exocyclic order, so a second pass drops those atoms.
    "Scaffold of the normal form" equals "normal form of the scaffold's own spelling" on the table of the tests; it is not promised
    in general.  There is no SMILES writer: the scaffold comes back as graph arrays and as a key.
    L <= 64; the refusals are mol_key()'s, with ValueError before anything is launched.
    Sequence: mdt::tokens_compact -> mdt::mol_graph -> mdt::mol_scaffold; with ``normalize=True`` mdt::mol_hydrogens ->
    mdt::mol_rings -> mdt::mol_normalize go between the last two."""
    (natoms, atoms, nbonds, bonds, atom_map, flags), status, position = _scaffold_of(tokens, vocabulary, device, normalize, exocyclic,
                                                                                      generic)
    return (natoms.long(), atoms.long() & 0xFFFFFFFF, nbonds.long(), bonds.long(), atom_map.long(), flags.long(), status.long(),
            position.long())


def scaffold_key(tokens, vocabulary: "SmilesVocabulary", device, *, normalize: bool = False, exocyclic: bool = True,
                 generic: bool = False):
    """mol_key() of the scaffold of each row (mol_scaffold(), whose keywords this takes; see there for what a scaffold is and is
    not -- not RDKit's MurckoScaffold) -> (key int64 (R,): the uint64 bits, flags int64 (R,), status int64 (R,), position int64
    (R,)).  Two molecules on one ring framework have one key whatever their side chains; KEY 0 MEANS "NO SCAFFOLD": no molecule, or
    an acyclic one.  ``flags`` are mol_scaffold()'s.  The key is mol_key()'s refinement hash, with its limits.
    Sequence: mol_scaffold()'s, then mdt::mol_key."""
    out, status, position = _scaffold_of(tokens, vocabulary, device, normalize, exocyclic, generic)
    return torch.ops.mdt.mol_key(*out[:4]), out[5].long(), status.long(), position.long()


# ----------------------------------------------------------------------------------------------------------------------
# graph rows back to token rows: the SMILES writer (csrc/k_molwrite.hip): rows of at most 64 atoms, written rows of at most 128 tokens
# ----------------------------------------------------------------------------------------------------------------------
def _width_arg(width, default: int) -> int:
    """The refusals of ``width=`` -> the width of the written rows."""
    if width is None:
        return default
    if isinstance(width, bool) or not isinstance(width, int) or not 1 <= width <= MAX_WRITE_WIDTH:
        raise ValueError(f"width must be an int in 1..{MAX_WRITE_WIDTH} or None, got {width!r} (wider rows are out of scope)")
    return width


def _invariant_arg(invariant) -> None:
    if not isinstance(invariant, bool):
        raise ValueError(f"invariant must be True or False, got {invariant!r}")


def _canonical_arg(canonical, invariant) -> None:
    if not isinstance(canonical, bool):
        raise ValueError(f"canonical must be True or False, got {canonical!r}")
    if canonical and not invariant:
        raise ValueError("canonical=True needs invariant=True: the canonical order is a priority, invariant=False writes as numbered")


def _write(graph, vocabulary, device, width, invariant, canonical=False):
    """mdt::mol_rank (only with ``invariant``) -> mdt::mol_write on device graph arrays; with ``canonical`` mdt::mol_canon goes
    between the two and its priority is taken wherever the row is decided (a torch.where on the flag: no synchronisation)"""
    priority = torch.ops.mdt.mol_rank(*graph) if invariant else None
    if canonical:
        searched, _, _, _, canon_flags = torch.ops.mdt.mol_canon(*graph)
        priority = torch.where((canon_flags == rt.MOLC_CANONICAL)[:, None], searched, priority)
    return torch.ops.mdt.mol_write(*graph, priority, vocabulary.class_id_on(torch.device(device)), width)


def mol_write(natoms, atoms, nbonds, bonds, vocabulary: "SmilesVocabulary", device, *, width: int, invariant: bool = True,
              canonical: bool = False):
    """Graph arrays back to SMILES token rows -> (tokens int64 (R, width), length int64 (R,), token_atom int64 (R, width), flags
    int64 (R,)).  The four graph arrays may come from any producer -- mol_graph(), mol_normalize(), mol_scaffold(), the ops behind
    them, or your own -- as integer tensors in mol_graph()'s format, (R,) counts and (R, L) words, L <= 64.

    ``tokens[r, :length[r]]`` spells row r in the ids of ``vocabulary`` (``vocabulary.decode`` gives the string), zero after;
    ``token_atom`` is 1 + the atom each token belongs to (an atom's text and its ring numbers; a bond symbol, '(' and ')' go with
    the atom they lead to), 0 for '.' and for padding.  ``flags``: 1 written; 2 the row needs ``length`` > ``width`` tokens; 4 the
    vocabulary lacks a character the row needs ('%' for a tenth open ring, '[' for a bracket atom, ...); 8 the arrays are not
    writable (an entry (a, a), a pair of atoms named by two entries, an order outside 1..5, an atom word no scan writes); 0 no
    molecule.  With anything but 1 the tokens are all zero.
    The walk is a depth-first one that takes start atoms and neighbours in ascending (priority, index), ring numbers from the
    lowest free one, bond symbols only where mol_graph() would read another order; mdt_mol_write in include/mdt_hip.h has every
    rule.  ``invariant=True`` takes the priority from the refinement behind mol_key() (one root per dotted component), so that
    the row depends on the numbering of the atoms only through ties the index then breaks: the four random spellings of each of
    the 500 graphs of the tests come out as one row.  ``invariant=False`` visits the atoms as numbered: a row written this way
    reads back to the same numbering.
    What it promises: mol_graph() of a written row whose unbracketed atoms pass smiles_check()'s valence rule has status 0, the
    same atom words in the order the atoms appear, the same bonds, hence the same mol_key().
    What it is NOT: NOT RDKit's canonical SMILES, and with ``canonical=False`` not a canonical form at all -- ties are broken by
    index, not by search, so two numberings of a symmetric molecule CAN give two rows (coronene does; none of the 30 molecules of
    the tests' symmetric table did).  ``canonical=True`` (needs ``invariant=True``) takes the priority from the search of
    mol_canon() instead: every row the search DECIDES is written the same way under every numbering of its atoms -- coronene gives
    one row.  A row the search leaves undecided (more than 4,096 nodes: hexaphenylethane) is written with the priority of
    ``canonical=False``; mol_canon() tells which rows those are.  THE COST: the search runs for every row, one wave a row, and
    has no automorphism pruning -- about 1.6 passes of mdt::mol_rank on rows of ordinary generated molecules, but a row that runs
    to the cap (hexaphenylethane) keeps its wave busy for about a second, alone on its compute unit, and a batch with many
    such cage-like rows has not been measured: ask mol_canon() for ``nodes`` on a sample first.  Still not promised: RDKit's canonical SMILES, stereo (the graph
    has none), a preferred Kekule structure (orders are written as handed in), undecided rows, rows wider than 128 tokens.
    Refused with ValueError before anything is launched: arrays that are not integer (R,) / (R, L) tensors of matching shapes,
    L > 64, ``width`` outside 1..128, ``canonical=True`` with ``invariant=False``.  Sequence: mdt::mol_rank (only with
    ``invariant=True``) -> mdt::mol_canon (only with ``canonical=True``) -> mdt::mol_write."""
    if not isinstance(vocabulary, SmilesVocabulary):
        raise ValueError(f"vocabulary must be a SmilesVocabulary, got {type(vocabulary).__name__}")
    _invariant_arg(invariant)
    _canonical_arg(canonical, invariant)
    if width is None:
        raise ValueError("width must be given: the graph arrays do not say how wide the rows were")
    width = _width_arg(width, 0)
    arrays = []
    for name, t in (("natoms", natoms), ("atoms", atoms), ("nbonds", nbonds), ("bonds", bonds)):
        if not isinstance(t, Tensor) or t.dtype not in (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8):
            raise ValueError(f"{name} must be an integer tensor")
        arrays.append(t)
    natoms, atoms, nbonds, bonds = arrays
    if atoms.dim() != 2 or bonds.shape != atoms.shape or natoms.shape != atoms.shape[:1] or nbonds.shape != atoms.shape[:1]:
        raise ValueError("atoms and bonds must be (R, L) with one natoms and one nbonds per row")
    if not 1 <= atoms.shape[1] <= MAX_MOL_LENGTH:
        raise ValueError(f"atoms has rows of {atoms.shape[1]} positions; the writer takes 1 to {MAX_MOL_LENGTH} "
                         "(wider rows are out of scope)")
    device = torch.device(device)
    graph = tuple(t.to(device).to(torch.int32) for t in (natoms, atoms, nbonds, bonds))   # (the low 32 bits: the words as written)
    tokens, length, token_atom, flags = _write(graph, vocabulary, device, width, invariant, canonical)
    return tokens.long(), length.long(), token_atom.long(), flags.long()


def mol_respell(tokens, vocabulary: "SmilesVocabulary", device, *, normalize: bool = False, invariant: bool = True, width=None,
                canonical: bool = False):
    """One spelling per molecule -> (tokens int64 (R, width), flags int64 (R,), status int64 (R,), position int64 (R,)) for raw
    (R, L) ids of any integer dtype, zeros anywhere: the graph behind each row (mol_graph()), written again by mol_write().  With
    ``invariant=True`` two rows that spell one graph -- another start atom, branch order, ring numbers, %nn, an explicit '-', the
    order of dotted components -- come back as the same row, so generated molecules can be stored and deduplicated as strings.
    ``normalize=True`` spells the normal form of mol_normalize(): every atom in brackets with its hydrogens, aromaticity as
    perceived there, so that [CH4] and C, c1ccccc1 and C1=CC=CC=C1 come back as one row (a much longer one).
    ``status`` / ``position`` are smiles_check()'s; ``flags`` are mol_write()'s: 1 written, 2 too long for ``width`` (default: the
    input's L), 4 the vocabulary lacks a character, 0 no molecule (status != 0 or empty); rows of flags != 1 are all zero.  108 of
    the 2,000 random spellings of the tests come back longer than they went in, none beyond 55 tokens.
    NOT RDKit's canonical SMILES, and by default not a canonical form: two numberings of a symmetric molecule can come back as two
    rows (coronene).  ``canonical=True`` (needs ``invariant=True``) takes the visiting order from the search of mol_canon(): every
    row the search decides comes back as ONE row under every numbering; an undecided row (more than 4,096 nodes) comes back as
    with ``canonical=False``.  The search costs about 1.6 passes of mdt::mol_rank on ordinary rows and up to about a second for
    ONE row that runs to the cap (no automorphism pruning; many such rows in a batch are unmeasured): see mol_write().  Not
    promised either way: RDKit's canonical SMILES, stereo, a preferred Kekule structure, undecided
    rows; see mol_write().
    L <= 64; the refusals are mol_key()'s, ``width`` outside 1..128 and ``canonical=True`` with ``invariant=False``, with
    ValueError before anything is launched.
    Sequence: mdt::tokens_compact -> mdt::mol_graph -> mdt::mol_rank (only with ``invariant=True``) -> mdt::mol_canon (only with
    ``canonical=True``) -> mdt::mol_write; with ``normalize=True`` mdt::mol_hydrogens -> mdt::mol_rings -> mdt::mol_normalize go
    after mdt::mol_graph."""
    _normalize_arg(normalize)
    _invariant_arg(invariant)
    _canonical_arg(canonical, invariant)
    tok = _integer_ids(tokens, "tokens")
    width = _width_arg(width, tok.shape[1])
    packed, n = _mol_rows(tok, vocabulary, device)
    graph, status, position = _graph_rows(packed, n, vocabulary, device, normalize)
    out, _, _, flags = _write(graph, vocabulary, device, width, invariant, canonical)
    return out.long(), flags.long(), status.long(), position.long()


def scaffold_tokens(tokens, vocabulary: "SmilesVocabulary", device, *, normalize: bool = False, exocyclic: bool = True,
                    generic: bool = False, width=None, canonical: bool = False):
    """The scaffold of each row as a row the model and a chemist can read -> (tokens int64 (R, width), flags int64 (R,),
    scaffold_flags int64 (R,), status int64 (R,), position int64 (R,)): mol_scaffold() (whose keywords this takes; see there for
    what a scaffold is and is not -- not RDKit's MurckoScaffold), written by mol_write() with ``invariant=True``, so that two
    decorations of one ring system give the same row.  ``flags`` are mol_write()'s (1 written; 0 for a row without a scaffold,
    whose tokens are all zero), ``scaffold_flags`` mol_scaffold()'s, ``status`` / ``position`` smiles_check()'s.  ``width``
    defaults to the input's L.  The spelling is NOT RDKit's canonical SMILES and by default not a canonical form; with
    ``canonical=True`` a scaffold whose search is decided has one row under every numbering (mol_write()).
    Sequence: mol_scaffold()'s, then mdt::mol_rank -> mdt::mol_canon (only with ``canonical=True``) -> mdt::mol_write."""
    _canonical_arg(canonical, True)
    tok = _integer_ids(tokens, "tokens")
    width = _width_arg(width, tok.shape[1])
    out, status, position = _scaffold_of(tok, vocabulary, device, normalize, exocyclic, generic)
    written, _, _, flags = _write(out[:4], vocabulary, device, width, True, canonical)
    return written.long(), flags.long(), out[5].long(), status.long(), position.long()


def scaffold_keep(tokens, vocabulary: "SmilesVocabulary", device, *, normalize: bool = False, exocyclic: bool = True, width=None,
                  canonical: bool = False):
    """A lead respelled, and the mask of its scaffold's tokens -> (tokens int64 (R, width), keep_mask bool (R, width), flags int64
    (R,), status int64 (R,), position int64 (R,)).  ``tokens`` is mol_respell()'s row (``invariant=True``; with ``normalize`` the
    normal form); ``keep_mask`` is True exactly at the tokens that belong to an atom of the scaffold (mol_scaffold() with the same
    ``normalize`` / ``exocyclic``): the atom's text, its ring numbers, and the bond symbol and parentheses that lead to it.  This is
    the mask refine_keep_tokens(keep_mask=) takes: refine a lead around its kept ring system.  A row without a scaffold, or one
    that was not written (``flags`` != 1), has an all-False mask.  What leads from a kept atom to a pruned one -- '(' , a bond
    symbol, ')' -- goes with the pruned atom and is not kept.
    The limits are mol_write()'s (NOT RDKit's canonical SMILES; ``canonical=True`` makes the respelled lead, and with it the mask,
    the same under every numbering of a lead whose search is decided) and mol_scaffold()'s (not RDKit's MurckoScaffold).
    Sequence: mdt::tokens_compact -> mdt::mol_graph -> mdt::mol_scaffold -> mdt::mol_rank -> mdt::mol_canon (only with
    ``canonical=True``) -> mdt::mol_write, with
    ``normalize=True`` mdt::mol_hydrogens -> mdt::mol_rings -> mdt::mol_normalize after mdt::mol_graph; the mask is torch on the
    two ops' outputs, no kernel of its own."""
    _normalize_arg(normalize)
    _canonical_arg(canonical, True)
    mode = _scaffold_mode(exocyclic, False)
    tok = _integer_ids(tokens, "tokens")
    width = _width_arg(width, tok.shape[1])
    packed, n = _mol_rows(tok, vocabulary, device)
    graph, status, position = _graph_rows(packed, n, vocabulary, device, normalize)
    atom_map = torch.ops.mdt.mol_scaffold(*graph, mode)[4]
    written, _, token_atom, flags = _write(graph, vocabulary, device, width, True, canonical)
    kept = torch.cat([torch.zeros_like(atom_map[:, :1]), atom_map], dim=1) != 0          # (R, 1 + L): column 0 is "no atom"
    keep_mask = torch.gather(kept, 1, token_atom.long())
    return written.long(), keep_mask, flags.long(), status.long(), position.long()


# ----------------------------------------------------------------------------------------------------------------------
# the canonical atom order (csrc/k_molcanon.hip): rows of at most 64 atoms, search trees of at most 4,096 nodes
# ----------------------------------------------------------------------------------------------------------------------
def _canon_rows(tokens, vocabulary, device, normalize):
    """mol_canon()'s launches on raw ids -> (the op's five outputs, the graph arrays, status, position)"""
    _normalize_arg(normalize)
    packed, n = _mol_rows(tokens, vocabulary, device)
    graph, status, position = _graph_rows(packed, n, vocabulary, device, normalize)
    return torch.ops.mdt.mol_canon(*graph), graph, status, position


def mol_canon(tokens, vocabulary: "SmilesVocabulary", device, *, normalize: bool = False):
    """The canonical atom order of each row -> (rank int64 (R, L), canon_atoms int64 (R, L), canon_bonds int64 (R, L), natoms int64
    (R,), nbonds int64 (R,), flags int64 (R,), nodes int64 (R,), status int64 (R,), position int64 (R,)) for raw (R, L) ids of any
    integer dtype, zeros anywhere: the graph behind each row (mol_graph(); with ``normalize=True`` its normal form,
    mol_normalize()) relabelled by an individualisation-refinement SEARCH over mol_key()'s refinement, the smallest relabelled graph
    as the answer.  ``rank[r, a]`` is 1 + the canonical position of atom a (0 beyond ``natoms``); ``canon_atoms`` are the atom words
    in canonical position, ``canon_bonds`` the entries lo | hi << 8 | order << 16 in canonical positions, ascending, zero beyond the
    counts.  ``flags``: 1 canonical; 2 undecided -- the search trees have more than 4,096 nodes (``nodes`` is then some value above
    that), the three arrays are all zero; 0 no molecule (status != 0 or empty).  Two rows of flags 1 are the same molecular graph
    EXACTLY when their counts, ``canon_atoms`` and ``canon_bonds`` are equal: the compare is on the relabelled graph itself, not on a
    hash (mol_same() does it).  There is no automorphism pruning: cubane takes 81 nodes, dodecahedrane 201, hexaphenylbenzene 1,531;
    hexaphenylethane (4,608 leaves) is undecided.  Not RDKit's canonical atom order; no stereo; orders are compared as written
    (c1ccccc1 and C1=CC=CC=C1 differ unless ``normalize=True``).
    L <= 64; the refusals are mol_key()'s, with ValueError before anything is launched.
    Sequence: mdt::tokens_compact -> mdt::mol_graph -> mdt::mol_canon; with ``normalize=True`` mdt::mol_hydrogens ->
    mdt::mol_rings -> mdt::mol_normalize go after mdt::mol_graph."""
    (rank, canon_atoms, canon_bonds, nodes, flags), graph, status, position = _canon_rows(tokens, vocabulary, device, normalize)
    return (rank, canon_atoms.long() & 0xFFFFFFFF, canon_bonds.long() & 0xFFFFFFFF, graph[0].long(), graph[2].long(), flags.long(), nodes.long(),
            status.long(), position.long())


def mol_same(a_tokens, b_tokens, vocabulary: "SmilesVocabulary", device, *, normalize: bool = False):
    """Are row r of ``a_tokens`` and row r of ``b_tokens`` the same molecular graph, exactly?  -> (same bool (R,), undecided bool
    (R,)) for raw ids of any integer dtype with the same number of rows (the widths may differ).  ``same`` compares the counts and
    the canonical arrays of mol_canon(), so it is an identity test, not a hash compare.  A pair with an undecided side is
    ``same = False, undecided = True``; two rows that are no molecule are not the same.
    The refusals are mol_canon()'s and a different number of rows, with ValueError before anything is launched.
    Sequence: mol_canon()'s for ``a_tokens``, then for ``b_tokens``; the compare is torch on the ops' outputs."""
    _normalize_arg(normalize)
    a, b = _integer_ids(a_tokens, "a_tokens"), _integer_ids(b_tokens, "b_tokens")
    if a.shape[0] != b.shape[0]:
        raise ValueError(f"a_tokens has {a.shape[0]} rows and b_tokens {b.shape[0]}: they are compared row by row")
    if not isinstance(vocabulary, SmilesVocabulary):
        raise ValueError(f"vocabulary must be a SmilesVocabulary, got {type(vocabulary).__name__}")
    for name, t in (("a_tokens", a), ("b_tokens", b)):           # (both are refused before the first launch)
        if not 1 <= t.shape[1] <= MAX_MOL_LENGTH:
            raise ValueError(f"{name} has rows of {t.shape[1]} positions; the canonical order takes 1 to {MAX_MOL_LENGTH} "
                             "(wider rows are out of scope)")
    (_, xa, xb, _, fa), ga, _, _ = _canon_rows(a, vocabulary, device, normalize)
    (_, ya, yb, _, fb), gb, _, _ = _canon_rows(b, vocabulary, device, normalize)
    width = max(xa.shape[1], ya.shape[1])
    pad = lambda t: torch.nn.functional.pad(t, (0, width - t.shape[1]))  # noqa: E731
    decided = (fa == rt.MOLC_CANONICAL) & (fb == rt.MOLC_CANONICAL)
    same = (decided & (ga[0] == gb[0]) & (ga[2] == gb[2]) & (pad(xa) == pad(ya)).all(dim=1) & (pad(xb) == pad(yb)).all(dim=1))
    return same, (fa == rt.MOLC_UNDECIDED) | (fb == rt.MOLC_UNDECIDED)


# ----------------------------------------------------------------------------------------------------------------------
# what do two molecules share?  maximum common substructure of row pairs (csrc/k_molmcs.hip): rows of at most 64 atoms a side
# ----------------------------------------------------------------------------------------------------------------------
MCS_ATOMS = ("element", "exact")


class McsResult(NamedTuple):
    """What mol_mcs() returns."""
    bonds: Tensor         # (R,) int64: the matched bonds
    atoms: Tensor         # (R,) int64: the matched atoms
    map_a: Tensor         # (R, LA) int64: 1 + the b atom that a atom x is matched with, 0 = none
    in_a: Tensor          # (R, LA) bool: a atom x is in the common substructure
    in_b: Tensor          # (R, LB) bool: b atom t is
    similarity: Tensor    # (R,) float64: shared atoms and bonds over the union of both sides' atoms and bonds
    undecided: Tensor     # (R,) bool: some root ran into the step cap: the result is a lower bound
    whole_a: Tensor       # (R,) bool: all of a is in it (a is a substructure of b; a row with a doubled bond: see mol_mcs())
    whole_b: Tensor       # (R,) bool: all of b is
    steps: Tensor         # (R,) int64: the steps of the search
    natoms: Tensor        # (R,) int64  \
    graph_atoms: Tensor   # (R, LA) int64  the common substructure as graph arrays of its own, mol_graph()'s format:
    nbonds: Tensor        # (R,) int64     what mol_write() and the ops behind mol_key() take
    graph_bonds: Tensor   # (R, LA) int64 /
    atom_map: Tensor      # (R, LA) int64: 1 + the index in those arrays of a atom x, 0 = not kept
    pair: Tensor          # (R,) bool: both rows are molecules
    a_status: Tensor      # (R,) int64, smiles_check()'s, of a_tokens
    a_position: Tensor    # (R,) int64
    b_status: Tensor      # (R or 1,) int64, of b_tokens
    b_position: Tensor    # (R or 1,) int64


def _mcs_rows(a_tokens, b_tokens, vocabulary, normalize, atoms, names=("a_tokens", "b_tokens")):
    """The refusals of the mol_mcs() family, before anything is launched -> (a ids, b ids, the mode of mdt::mol_mcs)"""
    _normalize_arg(normalize)
    if atoms not in MCS_ATOMS:
        raise ValueError(f"atoms must be one of {MCS_ATOMS}, got {atoms!r}")
    a, b = _integer_ids(a_tokens, names[0]), _integer_ids(b_tokens, names[1])
    if b.shape[0] != a.shape[0] and b.shape[0] != 1:
        raise ValueError(f"{names[0]} has {a.shape[0]} rows and {names[1]} {b.shape[0]}: they are compared row by row, or every "
                         f"row of {names[0]} against ONE row of {names[1]}")
    if not isinstance(vocabulary, SmilesVocabulary):
        raise ValueError(f"vocabulary must be a SmilesVocabulary, got {type(vocabulary).__name__}")
    for name, t in zip(names, (a, b)):                           # (both are refused before the first launch)
        if not 1 <= t.shape[1] <= MAX_MOL_LENGTH:
            raise ValueError(f"{name} has rows of {t.shape[1]} positions; the common substructure takes 1 to {MAX_MOL_LENGTH} "
                             "(wider rows are out of scope)")
    return a, b, rt.MCS_EXACT_ATOMS if atoms == "exact" else 0


def _mcs_of(a, b, vocabulary, device, normalize, mode):
    """The launches up to mdt::mol_mcs -> (its ten outputs, a's graph AS WRITTEN, a's and b's graphs as matched, both sides' status
    and position)"""
    packed, n = _mol_rows(a, vocabulary, device)
    written, a_status, a_position = _graph_rows(packed, n, vocabulary, device)
    ga = _normal_form(*written)[0] if normalize else written
    packed, n = _mol_rows(b, vocabulary, device)
    gb, b_status, b_position = _graph_rows(packed, n, vocabulary, device, normalize)
    return torch.ops.mdt.mol_mcs(*ga, *gb, mode), written, ga, gb, (a_status, a_position, b_status, b_position)


def _usable_entries(graph):
    """(R,) int64: the bond entries of each row whose ends differ and whose order is 1..5"""
    _, _, nbonds, bonds = graph
    w = bonds.long() & 0xFFFFFFFF
    listed = torch.arange(w.shape[1], device=w.device)[None, :] < nbonds.long()[:, None]
    order = w >> 16
    return (listed & ((w & 255) != ((w >> 8) & 255)) & (order >= 1) & (order <= 5)).sum(1)


def _mcs_in_b(map_a, LB: int):
    """(R, LA) int64 1 + partner -> (R, LB) bool: the b atoms that are some a atom's partner"""
    return torch.zeros(map_a.shape[0], 1 + LB, dtype=torch.bool, device=map_a.device).scatter_(1, map_a, True)[:, 1:]   # column 0: none


def mol_mcs(a_tokens, b_tokens, vocabulary: "SmilesVocabulary", device, *, normalize: bool = False, atoms: str = "element") -> McsResult:
    """What do row r of ``a_tokens`` and row r of ``b_tokens`` share, and where do they differ?  -> McsResult (see its fields) for
    raw ids of any integer dtype, zeros anywhere; ``b_tokens`` has as many rows as ``a_tokens`` or ONE row, against which every row
    of ``a_tokens`` is then held (a batch of candidates and their target).  The widths LA, LB <= 64 may differ.

    The answer is the MAXIMUM COMMON SUBSTRUCTURE of the two graphs of mol_graph(): the greatest connected subgraph of a that also
    lies in b, compared by (bonds, atoms), bonds first, as RDKit's FindMCS does by default -- the edge kind, not the induced kind:
    C1CC1 and CCC share 2 bonds and 3 atoms.  ``atoms="element"`` pairs atoms of the same symbol and aromatic bit (charges,
    hydrogens and isotopes are ignored); ``"exact"`` wants the whole atom word equal.  Bonds pair when their order is equal.
    ``map_a`` / ``in_a`` / ``in_b`` name the atoms in each row's own order of appearance; ``similarity`` is (atoms + bonds) / (a's
    atoms + bonds + b's atoms + bonds - atoms - bonds) from the exact integer counts, 1.0 exactly when each is all of the other, 0
    where the pair is no pair (``pair`` False: a row is no molecule; everything is then zero).  ``undecided``: a root of the search
    ran into its cap of 4096 steps, and the result is a valid common substructure and a LOWER bound, like FindMCS's ``canceled``.
    ``whole_a``: a is a substructure of b.  The graph arrays are the common substructure as a molecule of its own, a's atoms in a's
    order: mol_write() and the ops behind mol_key() take them as they are (mcs_tokens() writes them).
    The search -- roots, bound, greedy floor, cap -- is part of the definition; mdt_mol_mcs in include/mdt_hip.h has every step.
    What it is NOT: not RDKit's FindMCS -- no ring-matches-ring or complete-rings options, no SMARTS result, no stereo; the result is
    connected, so it is ONE fragment; aromaticity is as written unless ``normalize=True``, which compares the normal forms
    (mol_normalize()) and so molecules, not spellings.  Where ``undecided`` is False, sizes, ``similarity`` and the whole flags
    do not depend on how either row is spelled; which atoms are named can.  ONE EXCEPTION: a row that names one pair of atoms by
    two bonds (two ring closures between the same atoms, C12CC12: a row mol_write() calls not writable, about 1 % of mutated
    rows).  As ``a_tokens`` such a row can get a SMALLER common substructure than the greatest one without ``undecided``, and
    ``whole_a`` can then be False although a lies in b: the search's bound reads b's bonds as a set and a's one by one.
    The refusals are mol_same()'s, a ``b_tokens`` of neither R rows nor one, and ``atoms`` outside ("element", "exact"), with
    ValueError before anything is launched.  Sequence: mdt::tokens_compact -> mdt::mol_graph for ``a_tokens``, the same for
    ``b_tokens``, then mdt::mol_mcs; with ``normalize=True`` mdt::mol_hydrogens -> mdt::mol_rings -> mdt::mol_normalize go after
    each mdt::mol_graph.  The rest is torch on the op's outputs."""
    a, b, mode = _mcs_rows(a_tokens, b_tokens, vocabulary, normalize, atoms)
    out, _, ga, gb, (a_status, a_position, b_status, b_position) = _mcs_of(a, b, vocabulary, device, normalize, mode)
    size, map_a, _, steps, natoms, graph_atoms, nbonds, graph_bonds, atom_map, flags = out
    map_a, flags = map_a.long(), flags.long()
    in_b = _mcs_in_b(map_a, b.shape[1])
    pair = (flags & rt.MCS_PAIR) != 0
    common = size.long().sum(1)
    union = ga[0].long() + _usable_entries(ga) + gb[0].long() + _usable_entries(gb) - common
    similarity = torch.where(pair, common.double() / union.clamp(min=1).double(), torch.zeros_like(common, dtype=torch.float64))
    return McsResult(size[:, 0].long(), size[:, 1].long(), map_a, map_a != 0, in_b, similarity, (flags & rt.MCS_UNDECIDED) != 0,
                     (flags & rt.MCS_WHOLE_A) != 0, (flags & rt.MCS_WHOLE_B) != 0, steps.long(), natoms.long(),
                     graph_atoms.long() & 0xFFFFFFFF, nbonds.long(), graph_bonds.long(), atom_map.long(), pair, a_status.long(),
                     a_position.long(), b_status.long(), b_position.long())


def mol_difference(a_tokens, b_tokens, vocabulary: "SmilesVocabulary", device, *, normalize: bool = False, atoms: str = "element"):
    """Where do two molecules differ?  -> (only_a bool (R, LA), only_b bool (R, LB), undecided bool (R,)): the atoms of each row
    OUTSIDE the maximum common substructure of mol_mcs() (whose arguments and limits this takes), in each row's own order of
    appearance -- the two highlight lists of the reference's view_difference(), as masks.  Positions beyond a row's atoms are
    False, as is everything in a pair that is no pair.  Sequence: mol_mcs()'s."""
    a, b, mode = _mcs_rows(a_tokens, b_tokens, vocabulary, normalize, atoms)
    out, _, ga, gb, _ = _mcs_of(a, b, vocabulary, device, normalize, mode)
    map_a, flags = out[1].long(), out[9].long()
    in_b = _mcs_in_b(map_a, b.shape[1])
    pair = ((flags & rt.MCS_PAIR) != 0)[:, None]
    inside_a = torch.arange(a.shape[1], device=map_a.device)[None, :] < ga[0].long()[:, None]
    inside_b = torch.arange(b.shape[1], device=map_a.device)[None, :] < gb[0].long()[:, None]       # (R or 1, LB)
    return inside_a & (map_a == 0) & pair, inside_b & ~in_b & pair, (flags & rt.MCS_UNDECIDED) != 0


def mcs_tokens(a_tokens, b_tokens, vocabulary: "SmilesVocabulary", device, *, normalize: bool = False, atoms: str = "element",
               width=None, canonical: bool = False):
    """The maximum common substructure of each pair as a row the model and a chemist can read -> (tokens int64 (R, width), flags
    int64 (R,), undecided bool (R,), a_status int64 (R,), b_status int64 (R or 1,)): the graph arrays of mol_mcs() (whose
    arguments and limits this takes) written by mol_write() with ``invariant=True``.  ``flags`` are mol_write()'s (1 written; 0
    where nothing is shared, the tokens are then all zero).  ``width`` defaults to the LA of ``a_tokens``; ``canonical`` as on
    scaffold_tokens().  The atoms are a's, with a's words: a bracket atom keeps its H count, an unbracketed atom that lost a
    neighbour reads as carrying more implicit hydrogens -- the row is a fragment to look at, not a reaction product.  mol_key() of
    the written row is mdt::mol_key of the graph arrays.  NOT RDKit's canonical SMILES and not FindMCS's SMARTS.
    Sequence: mol_mcs()'s, then mdt::mol_rank -> mdt::mol_canon (only with ``canonical=True``) -> mdt::mol_write."""
    _canonical_arg(canonical, True)
    a, b, mode = _mcs_rows(a_tokens, b_tokens, vocabulary, normalize, atoms)
    width = _width_arg(width, a.shape[1])
    out, _, _, _, (a_status, _, b_status, _) = _mcs_of(a, b, vocabulary, device, normalize, mode)
    written, _, _, flags = _write(out[4:8], vocabulary, device, width, True, canonical)
    return written.long(), flags.long(), (out[9].long() & rt.MCS_UNDECIDED) != 0, a_status.long(), b_status.long()


def mcs_keep(lead_tokens, other_tokens, vocabulary: "SmilesVocabulary", device, *, normalize: bool = False, atoms: str = "element",
             width=None, canonical: bool = False):
    """A lead respelled, and the mask of the tokens it shares with another molecule -> (tokens int64 (R, width), keep_mask bool (R,
    width), complete bool (R,), flags int64 (R,), status int64 (R,), position int64 (R,)): "keep what this lead has in common with
    that molecule, vary the rest".  Shaped like substructure_keep(): ``tokens`` is the lead respelled (mol_write() with
    ``invariant=True``, ``width`` default the lead's L, ``canonical`` as there); ``keep_mask`` is True exactly at the tokens that
    belong to a lead atom inside the maximum common substructure of mol_mcs() with ``other_tokens`` (R rows, or one row for every
    lead) -- the atom's text, its ring numbers, and the bond symbol and parentheses that lead to it -- and is the mask
    refine_keep_tokens(keep_mask=) takes.  ``complete[r]`` is False where a root ran into the step cap: the kept part is a common
    substructure, but a greater one may exist.  A row that was not written (``flags`` != 1, mol_write()'s) or a pair that is no
    pair has an all-False mask; ``status`` / ``position`` are the lead's.
    ``normalize=True``: the match reads the normal forms of both sides, but the lead is written from the graph AS WRITTEN, as
    substructure_keep() does -- mol_normalize() keeps the atom numbering, so the matched atoms name the same tokens.
    The limits are mol_mcs()'s (not RDKit's FindMCS; connected; a step cap; no stereo) and mol_write()'s (NOT RDKit's canonical
    SMILES).  The refusals are mol_mcs()'s and ``width`` outside 1..128.
    Sequence: mdt::tokens_compact -> mdt::mol_graph for the lead, the same for the other, mdt::mol_mcs, then mdt::mol_rank ->
    mdt::mol_canon (only with ``canonical=True``) -> mdt::mol_write on the lead's graph; with ``normalize=True``
    mdt::mol_hydrogens -> mdt::mol_rings -> mdt::mol_normalize go after each mdt::mol_graph; the mask is torch on the ops' outputs,
    no kernel of its own."""
    _canonical_arg(canonical, True)
    a, b, mode = _mcs_rows(lead_tokens, other_tokens, vocabulary, normalize, atoms, ("lead_tokens", "other_tokens"))
    width = _width_arg(width, a.shape[1])
    out, lead, _, _, (status, position, _, _) = _mcs_of(a, b, vocabulary, device, normalize, mode)
    written, _, token_atom, flags = _write(lead, vocabulary, device, width, True, canonical)
    kept = torch.cat([torch.zeros_like(out[1][:, :1]), out[1]], dim=1) != 0              # (R, 1 + L): column 0 is "no atom"
    keep_mask = torch.gather(kept, 1, token_atom.long())
    return written.long(), keep_mask, (out[9].long() & rt.MCS_UNDECIDED) == 0, flags.long(), status.long(), position.long()


# ----------------------------------------------------------------------------------------------------------------------
# edit distance between molecules (csrc/k_edit.hip): rows of at most 64 positions, ids in [0, 64)
# ----------------------------------------------------------------------------------------------------------------------
def edit_distance(a_tokens, b_tokens, device) -> Tensor:
    """The Levenshtein distance (insert, delete, substitute: 1 each) between the molecules of ``a_tokens`` and ``b_tokens``, row by
    row: int64 (R,).  Both are raw (R, L) ids of any integer dtype and the same shape, zeros anywhere -- a molecule is its compacted
    id row, as in screen_tokens.  L <= 64 and ids in [0, 64) (one 64-bit word per pair; wider rows are out of scope), refused
    with ValueError before anything is launched.  Sequence: mdt::tokens_compact twice -> mdt::edit_distance."""
    a, b = _integer_ids(a_tokens, "a_tokens"), _integer_ids(b_tokens, "b_tokens")
    if tuple(a.shape) != tuple(b.shape):
        raise ValueError(f"a_tokens {tuple(a.shape)} and b_tokens {tuple(b.shape)} must have the same shape")
    if a.shape[1] < 1:
        raise ValueError("a_tokens must hold at least one position per row")
    _edit_width(a.shape[1], "a_tokens")
    a, b = _edit_ids(a, "a_tokens"), _edit_ids(b, "b_tokens")
    device = torch.device(device)
    ap, al, _, _ = torch.ops.mdt.tokens_compact(a.to(device), 0, 1.0)
    bp, bl, _, _ = torch.ops.mdt.tokens_compact(b.to(device), 0, 1.0)
    return torch.ops.mdt.edit_distance(ap, al, bp, bl).long()


def nearest_known(tokens, known_tokens, device):
    """How far from the known set is each molecule?  -> (distance int64 (R,), index int64 (R,)): the smallest Levenshtein distance
    of row r of ``tokens`` (raw (R, L) ids) to any molecule of ``known_tokens`` -- a KnownSet, or raw ids, wrapped as screen_tokens
    does -- and the lowest row of ``KnownSet.packed`` that attains it.  The result does not depend on how the device splits the
    work.  L <= 64 and ids in [0, 64), in both (wider rows are out of scope); an empty known set has no nearest: all refused with
    ValueError before anything is launched.  Sequence: mdt::tokens_compact -> mdt::edit_nearest."""
    tok = _integer_ids(tokens, "tokens")
    length = tok.shape[1]
    if length < 1:
        raise ValueError("tokens must hold at least one position per row")
    _edit_width(length, "tokens")
    known = known_tokens if isinstance(known_tokens, KnownSet) else KnownSet(known_tokens, length)
    if known.width != length:
        raise ValueError(f"known_tokens was built for rows of {known.width} positions, tokens has {length}")
    if len(known) == 0:
        raise ValueError("known_tokens is empty: there is no nearest known molecule")
    _edit_known(known)
    tok = _edit_ids(tok, "tokens")
    device = torch.device(device)
    packed, n, _, _ = torch.ops.mdt.tokens_compact(tok.to(device), 0, 1.0)
    _, kp, kl = known.on(device)
    dist, index = torch.ops.mdt.edit_nearest(packed, n, kp, kl)
    return dist.long(), index.long()


def screen_candidates(model: "QMDiffusion", model_forward: "QMDiffusionForward", conditioning: Tensor, device, candidates: int,
                      keep: int, *, cond_scale=1.0, timesteps: int = 100, noise=None, **screen_tokens_kwargs) -> Screened:
    """Best-of-N per target as one call: ``model.sample_tokens(conditioning.repeat(N, 1), ...)`` -- N = ``candidates`` tries for each
    of the G targets in one fused sampling call of N * G rows -- then screen_tokens (whose keyword arguments this takes, and
    ``min_distance`` / ``min_novelty`` / ``vocabulary`` / ``identity`` / ``max_similarity`` / ``max_known_similarity`` /
    ``fingerprint_radius`` / ``require`` / ``forbid`` / ``kekulize`` / ``limits`` / ``normalize`` / ``max_per_scaffold`` /
    ``novel_scaffold`` / ``scaffold_exocyclic`` / ``scaffold_generic`` / ``counts``, with which the tokens go to screen_tokens_diverse instead;
    ``sampler`` / ``sigma_schedule`` go to both models, as in generate_and_validate).  ``cond_scale``: one float, or N values, one per
    candidate block (expanded with repeat_interleave(G) into the per-sample guidance).  ``noise``: as sample_tokens; with
    ``noise=NoiseSource(seed=..., sample0=s)`` candidate block c is the scalar call whose sample0 is s + c * G (bit for bit under a
    pinned ``kernel_choice``)."""
    extra = set(screen_tokens_kwargs) - {"known_tokens", "weights", "forward_timesteps", "X_norm_factor", "forward_noise", "sampler",
                                         "sigma_schedule", "min_distance", "min_novelty", "vocabulary", "identity", "max_similarity",
                                         "max_known_similarity", "fingerprint_radius", "require", "forbid", "kekulize", "limits", "normalize",
                                         "max_per_scaffold", "novel_scaffold", "scaffold_exocyclic", "scaffold_generic", "counts"}
    if extra:
        raise TypeError(f"screen_candidates got unexpected keyword arguments {sorted(extra)}")
    _, known = _screen_args(conditioning, candidates, keep, screen_tokens_kwargs.get("known_tokens"),
                            screen_tokens_kwargs.get("weights"), length=model.max_length)
    if known is not None:
        screen_tokens_kwargs["known_tokens"] = known
    filters = dict(min_distance=screen_tokens_kwargs.pop("min_distance", 1), min_novelty=screen_tokens_kwargs.pop("min_novelty", 1))
    diverse = _diverse_args(filters["min_distance"], filters["min_novelty"], known, model.max_length)
    vocabulary = screen_tokens_kwargs.pop("vocabulary", None)
    _vocabulary_arg(vocabulary, model.max_length)
    if vocabulary is not None:
        diverse, filters["vocabulary"] = True, vocabulary
    identity = screen_tokens_kwargs.pop("identity", "string")
    _identity_arg(identity, vocabulary, model.max_length)
    if identity != "string":                                     # ("string": the calls made without the keyword)
        diverse, filters["identity"] = True, identity
    similar = {k: screen_tokens_kwargs.pop(k) for k in ("max_similarity", "max_known_similarity", "fingerprint_radius")
               if k in screen_tokens_kwargs}
    if any(similar.get(k) is not None for k in ("max_similarity", "max_known_similarity")):     # (both None: the calls made without)
        _similarity_args(similar.get("max_similarity"), similar.get("max_known_similarity"), similar.get("fingerprint_radius", 2),
                         vocabulary, known, model.max_length)
        diverse = True
        filters.update(similar)
    fragments = {k: screen_tokens_kwargs.pop(k) for k in ("require", "forbid") if k in screen_tokens_kwargs}
    fragments = {k: f for k, f in fragments.items() if f is not None}                         # (None: the calls made without)
    if fragments:
        _substructure_args(fragments.get("require"), fragments.get("forbid"), vocabulary, model.max_length)
        diverse = True
        filters.update(fragments)
    kekulize = screen_tokens_kwargs.pop("kekulize", False)
    _kekulize_arg(kekulize, vocabulary, model.max_length)
    if kekulize:                                                 # (False: the calls made without the keyword)
        diverse, filters["kekulize"] = True, True
    limits = screen_tokens_kwargs.pop("limits", None)
    _limits_arg(limits, vocabulary, model.max_length)
    if limits is not None:                                       # (None: the calls made without the keyword)
        diverse, filters["limits"] = True, limits
    scaffold = {k: screen_tokens_kwargs.pop(k) for k in ("max_per_scaffold", "novel_scaffold", "scaffold_exocyclic", "scaffold_generic")
                if k in screen_tokens_kwargs}
    scaffold_on = _scaffold_args(scaffold.get("max_per_scaffold"), scaffold.get("novel_scaffold", False),
                                 scaffold.get("scaffold_exocyclic", True), scaffold.get("scaffold_generic", False), vocabulary, known,
                                 model.max_length) is not None
    if scaffold_on:                                              # (None and False: the calls made without the keywords)
        diverse = True
        filters.update(scaffold)
    counts = screen_tokens_kwargs.pop("counts", None)
    _counts_arg(counts, vocabulary, model.max_length)
    if counts is not None:                                       # (None: the calls made without the keyword)
        diverse, filters["counts"] = True, counts
    normalize = screen_tokens_kwargs.pop("normalize", False)
    _screen_normalize_arg(normalize, vocabulary, model.max_length, identity == "graph" or bool(fragments) or scaffold_on or
                          counts is not None or any(
        similar.get(k) is not None for k in ("max_similarity", "max_known_similarity")))
    if normalize:                                                # (False: the calls made without the keyword)
        diverse, filters["normalize"] = True, True
    N, G = candidates, conditioning.shape[0]
    scale = guidance_rows(cond_scale, N, "cond_scale")
    if isinstance(scale, Tensor):
        scale = scale.repeat_interleave(G)
    tokens = model.sample_tokens(conditioning.repeat(N, 1), device, cond_scale=scale, timesteps=timesteps, noise=noise,
                                 sampler=screen_tokens_kwargs.get("sampler"), sigma_schedule=screen_tokens_kwargs.get("sigma_schedule"))
    if diverse:
        return screen_tokens_diverse(model_forward, tokens, conditioning, device, candidates, keep, **filters, **screen_tokens_kwargs)
    return screen_tokens(model_forward, tokens, conditioning, device, candidates, keep, **screen_tokens_kwargs)
