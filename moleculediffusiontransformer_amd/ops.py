"""`torch.ops.mdt.*`: the path's native entry points as PyTorch custom ops (last row).

Each op is a thin body over the C ABI of libmdt_hip.so (include/mdt_hip.h): tensors in, tensors out, launched on the
CURRENT HIP stream of the tensors' device, no hidden state besides the packed-weight handle a model owns (`handle`, an
integer from register_engine()).  Errors follow the TORCH_CHECK convention: every failure is a Python RuntimeError
(non-HIP tensors included -- there is no CPU implementation behind these ops; only shape inference is registered for
fake / meta tensors).

    cond_embed          generative.py:838-850 (fc1 -> GELU, PositionalEncoding1D, cat)
    precond_in / _out   KDiffusion_mod.denoise_fn scaling + clip (diffusion.py:798-814)
    cfg_mix             UNetCFG1d.forward guidance mix (modules.py:1253)
    cfg_mix_rows        the mix with one guidance scale per sample (a sample at scale 1 keeps its conditional prediction)
    adpm2_mid / _next   the two halves of ADPM2Sampler.step (diffusion.py:502-515)
    adpm2_euler         one Euler move of the step for a caller-supplied denoiser
    argmax_tokens       decode step after the path (generative.py:1212-1213)
    tokens_compact      ids -> non-zero ids left-packed, length, 64-bit key, forward input (generative.py:425-429 on ids)
    screen_score        weighted mean squared distance of re-predicted properties from the group's target
    screen_select       status (empty / non-finite / duplicate / known: is_novel, generative.py:1063) and the K best per group
    screen_select_diverse   the same with novelty as an edit distance and the K best that lie min_distance edits apart
    screen_select_reject / screen_select_diverse_reject   the two selections with a per-row `reject` byte OR-ed into the status
    smiles_check        well-formedness and valence of compacted id rows: status 0 / 32 / 64 and a position (csrc/k_smiles.hip)
    mol_graph / mol_key / key_flags   the molecular graph behind a row, its spelling-invariant 64-bit key, and the duplicate / known
                        flags by that key (csrc/k_molgraph.hip)
    mol_rank / mol_write   graph arrays back to token rows: a numbering-invariant visiting priority per atom, and the SMILES writer
                        that walks in its order (csrc/k_molwrite.hip)
    mol_canon           the canonical atom order of graph arrays by an individualisation-refinement search: the priority that
                        makes mol_write's row the same under every numbering, and the relabelled arrays (csrc/k_molcanon.hip)
    edit_distance       Levenshtein distance between compacted id rows, row by row (csrc/k_edit.hip)
    edit_nearest        per row the nearest row of a known set: its distance and its (lowest) index
    unet_eval           UNetCFG1d.forward: net(x, time, embedding=, embedding_scale=) (modules.py:1228-1255)
    aeuler_next         the whole AEulerSampler.step after its evaluation (diffusion.py:465-474)
    karras_hat / _mid / _next   the three stages of KarrasSampler.step (diffusion.py:417-435)
    sample              DiffusionSampler.forward + ADPM2Sampler.forward, the whole loop (diffusion.py:577-591, :517-524)
    sample_with         the same with the sampler chosen: ADPM2Sampler, AEulerSampler (:476-483) or KarrasSampler (:437-453)
    inpaint_tokens      DiffusionInpainter.forward + ADPM2Sampler.inpaint on a draft of token ids, decoded (diffusion.py:526-549, :612-625)
    refine_tokens       noise a draft of token ids up to the level of step k and run the remaining sampler steps, k per sample, decoded
    refine_keep_tokens  the same around a kept scaffold: a bool keep mask is re-noised from the draft in front of every step and held exactly
    all_gather_samples  the one collective of a sharded call (RCCL all_gather_into_tensor)
    precond_in_rows / precond_out_rows   the denoise scaling with ONE coefficient per sample (denoise_fn(sigmas=(B,)))
    unet_eval_rows      net(x, time=(B,), ...) as ONE evaluation: one time-mapping / FiLM row per sample
    eval_loss           KDiffusion_mod.forward's value per sample (diffusion.py:820-844): noising, one per-row evaluation, fused loss
"""
from __future__ import annotations

import weakref
from typing import Dict, Optional, Sequence, Tuple

import torch
from torch.library import custom_op

from . import runtime as rt
from .diffusion import (FUSED_SAMPLERS, ADPM2Sampler, NoiseSource, require_fused_kind, run_adpm2_inpaint, run_refine,
                        run_sampler)

Tensor = torch.Tensor

_ENGINES: "weakref.WeakValueDictionary[int, object]" = weakref.WeakValueDictionary()
_NEXT = [1]


def register_engine(engine) -> int:
    """Integer handle of a UNetEngine (packed weights + programs) for the ops that evaluate the network."""
    h = getattr(engine, "_op_handle", None)
    if h is None:
        h = _NEXT[0]
        _NEXT[0] += 1
        engine._op_handle = h
    _ENGINES[h] = engine
    return h


def _engine(handle: int):
    e = _ENGINES.get(handle)
    if e is None:
        raise RuntimeError(f"mdt: unknown or released engine handle {handle}")
    return e


def _engine_on(handle: int, dev, what: str):
    """The engine of ``handle``, which must live on the tensors' device ``dev``; ``what`` names the op in the message."""
    eng = _engine(handle)
    if eng.device != dev:
        raise RuntimeError(f"{what}: engine lives on {eng.device}, tensors on {dev}")
    return eng


def _hip(*tensors: Optional[Tensor]) -> torch.device:
    """Device guard: every tensor on ONE HIP device, fp32 unless stated; returns the device."""
    dev = None
    for t in tensors:
        if t is None:
            continue
        if t.device.type != "cuda":
            raise RuntimeError(f"mdt ops run on an AMD GPU through libmdt_hip.so; got a tensor on '{t.device}' "
                               "(there is no CPU implementation)")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError(f"mdt: tensors on different devices ({dev} and {t.device})")
    if dev is None:
        raise RuntimeError("mdt: no tensor argument")
    return dev


def _f32c(t: Tensor) -> Tensor:
    return t.detach().to(torch.float32).contiguous()


# ----------------------------------------------------------------------------------------------------------------------
@custom_op("mdt::cond_embed", mutates_args=())
def cond_embed(seq: Tensor, fc1_w: Tensor, fc1_b: Tensor, inv_freq: Optional[Tensor], pos_dim: int, pos_add: bool = False) -> Tensor:
    """pos_add: the positional encoding is added to the fc1 features (pos_emb_fourier_add) instead of concatenated."""
    dev = _hip(seq, fc1_w, fc1_b, inv_freq)
    lib = rt.load_library()
    seq, w, b = _f32c(seq), _f32c(fc1_w).view(-1), _f32c(fc1_b)
    B, n = seq.shape
    D1 = b.numel()
    if pos_dim and (inv_freq is None or inv_freq.numel() * 2 != pos_dim):
        raise RuntimeError("mdt::cond_embed: inv_freq must hold pos_dim / 2 frequencies")
    if pos_add and D1 > pos_dim:
        raise RuntimeError("mdt::cond_embed: the additive form needs text_embed_dim <= embed_dim_position (the encoding has "
                           "embed_dim_position columns, of which the first text_embed_dim are added)")
    inv = _f32c(inv_freq) if pos_dim else w
    out = torch.empty(B, n, D1 if pos_add else D1 + pos_dim, device=dev)
    if B:
        with torch.cuda.device(dev):
            if pos_add:
                rt.check(lib.mdt_cond_embed_add(rt.ptr(seq), rt.ptr(w), rt.ptr(b), rt.ptr(inv), rt.ptr(out), B, n, D1, pos_dim,
                                                rt.current_stream()))
            else:
                rt.check(lib.mdt_cond_embed(rt.ptr(seq), rt.ptr(w), rt.ptr(b), rt.ptr(inv), rt.ptr(out), B, n, D1, pos_dim,
                                            rt.current_stream()))
    return out


@cond_embed.register_fake
def _(seq, fc1_w, fc1_b, inv_freq, pos_dim, pos_add=False):
    return seq.new_empty(seq.shape[0], seq.shape[1], fc1_b.numel() + (0 if pos_add else pos_dim), dtype=torch.float32)


@custom_op("mdt::precond_in", mutates_args=())
def precond_in(x: Tensor, c_in: float, Cp: int) -> Tensor:
    dev = _hip(x)
    lib = rt.load_library()
    x = _f32c(x)
    B, C, L = x.shape
    if Cp < C or Cp % 16:
        raise RuntimeError(f"mdt::precond_in: Cp={Cp} must be a multiple of 16 and >= C={C}")
    out = torch.zeros(B, L, Cp, device=dev)
    if B:
        with torch.cuda.device(dev):
            rt.check(lib.mdt_precond_in(rt.ptr(x), rt.ptr(out), float(c_in), B, C, L, Cp, rt.current_stream()))
    return out


@precond_in.register_fake
def _(x, c_in, Cp):
    return x.new_empty(x.shape[0], x.shape[2], Cp, dtype=torch.float32)


def _dyn_scale(lib, x: Tensor, pred: Tensor, c_skip: float, c_out: float, q: float) -> Optional[Tensor]:
    """clip()'s per-sample dynamic threshold (diffusion.py:78-85) for the denoise stage of the next kernel, or None for q == 0."""
    if not q:
        return None
    B, C, L = x.shape
    scale = torch.empty(B, device=x.device)
    rt.check(lib.mdt_dyn_scale(rt.ptr(x), rt.ptr(pred), rt.ptr(scale), float(c_skip), float(c_out), float(q), B, C, L,
                               pred.shape[2], rt.current_stream()))
    return scale


@custom_op("mdt::precond_out", mutates_args=())
def precond_out(x: Tensor, pred: Tensor, c_skip: float, c_out: float, dynamic_threshold: float = 0.0) -> Tensor:
    """D = clip(c_skip x + c_out pred, dynamic_threshold) (diffusion.py:811-814, :75-88)."""
    dev = _hip(x, pred)
    lib = rt.load_library()
    x, pred = _f32c(x), _f32c(pred)
    B, C, L = x.shape
    if pred.dim() != 3 or pred.shape[0] != B or pred.shape[1] != L or pred.shape[2] < C:
        raise RuntimeError(f"mdt::precond_out: pred {tuple(pred.shape)} is not token-major (B, L, Cp) for x {tuple(x.shape)}")
    out = torch.empty_like(x)
    if B:
        with torch.cuda.device(dev):
            ds = _dyn_scale(lib, x, pred, c_skip, c_out, dynamic_threshold)
            rt.check(lib.mdt_precond_out(rt.ptr(x), rt.ptr(pred), rt.ptr(out), float(c_skip), float(c_out), B, C, L,
                                         pred.shape[2], rt.ptr(ds), rt.current_stream()))
    return out


@precond_out.register_fake
def _(x, pred, c_skip, c_out, dynamic_threshold=0.0):
    return x.new_empty(x.shape, dtype=torch.float32)


@custom_op("mdt::cfg_mix", mutates_args=())
def cfg_mix(cond: Tensor, uncond: Tensor, scale: float) -> Tensor:
    dev = _hip(cond, uncond)
    lib = rt.load_library()
    cond, uncond = _f32c(cond), _f32c(uncond)
    if cond.shape != uncond.shape:
        raise RuntimeError("mdt::cfg_mix: shape mismatch")
    out = torch.empty_like(cond)
    if cond.numel():
        with torch.cuda.device(dev):
            rt.check(lib.mdt_cfg_mix(rt.ptr(cond), rt.ptr(uncond), rt.ptr(out), float(scale), cond.numel(), rt.current_stream()))
    return out


@cfg_mix.register_fake
def _(cond, uncond, scale):
    return cond.new_empty(cond.shape, dtype=torch.float32)


@custom_op("mdt::cfg_mix_rows", mutates_args=())
def cfg_mix_rows(cond: Tensor, uncond: Tensor, scale: Tensor) -> Tensor:
    """cfg_mix with one scale per sample: scale holds cond.shape[0] values; a sample at scale 1 is its cond bit for bit."""
    dev = _hip(cond, uncond, scale)
    lib = rt.load_library()
    cond, uncond, scale = _f32c(cond), _f32c(uncond), _f32c(scale).flatten()
    if cond.shape != uncond.shape:
        raise RuntimeError("mdt::cfg_mix_rows: shape mismatch")
    if cond.dim() < 1 or scale.numel() != cond.shape[0]:
        raise RuntimeError(f"mdt::cfg_mix_rows: scale holds {scale.numel()} values for cond {tuple(cond.shape)}")
    out = torch.empty_like(cond)
    if cond.numel():
        with torch.cuda.device(dev):
            rt.check(lib.mdt_cfg_mix_rows(rt.ptr(cond), rt.ptr(uncond), rt.ptr(out), rt.ptr(scale), cond.shape[0],
                                          cond.numel() // cond.shape[0], rt.current_stream()))
    return out


@cfg_mix_rows.register_fake
def _(cond, uncond, scale):
    if cond.shape != uncond.shape:
        raise RuntimeError("mdt::cfg_mix_rows: shape mismatch")
    if cond.dim() < 1 or scale.numel() != cond.shape[0]:
        raise RuntimeError(f"mdt::cfg_mix_rows: scale holds {scale.numel()} values for cond {tuple(cond.shape)}")
    return cond.new_empty(cond.shape, dtype=torch.float32)


@custom_op("mdt::adpm2_mid", mutates_args=())
def adpm2_mid(x: Tensor, pred: Tensor, c_skip: float, c_out: float, sigma: float, dt_mid: float,
              c_in_mid: float, dynamic_threshold: float = 0.0) -> Tuple[Tensor, Tensor]:
    dev = _hip(x, pred)
    lib = rt.load_library()
    x, pred = _f32c(x), _f32c(pred)
    B, C, L = x.shape
    Cp = pred.shape[2]
    x_mid = torch.empty_like(x)
    xin = torch.zeros(B, L, Cp, device=dev)
    if B:
        with torch.cuda.device(dev):
            ds = _dyn_scale(lib, x, pred, c_skip, c_out, dynamic_threshold)
            rt.check(lib.mdt_adpm2_mid(rt.ptr(x), rt.ptr(pred), rt.ptr(x_mid), rt.ptr(xin), float(c_skip), float(c_out),
                                       float(sigma), float(dt_mid), float(c_in_mid), B, C, L, Cp, rt.ptr(ds), rt.current_stream()))
    return x_mid, xin


@adpm2_mid.register_fake
def _(x, pred, c_skip, c_out, sigma, dt_mid, c_in_mid, dynamic_threshold=0.0):
    return x.new_empty(x.shape, dtype=torch.float32), pred.new_empty(pred.shape, dtype=torch.float32)


@custom_op("mdt::adpm2_next", mutates_args=())
def adpm2_next(x: Tensor, x_mid: Tensor, pred: Tensor, noise: Optional[Tensor], c_skip: float, c_out: float,
               sigma_mid: float, dt_down: float, sigma_up: float, c_in_next: float, seed: int, step: int,
               sample0: int, dynamic_threshold: float = 0.0) -> Tuple[Tensor, Tensor]:
    """Returns (x_next, xin_next); noise None = counter-based generator keyed by (seed, step, sample0 + b)."""
    dev = _hip(x, x_mid, pred, noise)
    lib = rt.load_library()
    xn, x_mid, pred = _f32c(x).clone(), _f32c(x_mid), _f32c(pred)
    nz = None if noise is None else _f32c(noise)
    B, C, L = xn.shape
    Cp = pred.shape[2]
    xin = torch.zeros(B, L, Cp, device=dev)
    if B:
        with torch.cuda.device(dev):
            ds = _dyn_scale(lib, x_mid, pred, c_skip, c_out, dynamic_threshold)
            rt.check(lib.mdt_adpm2_next(rt.ptr(xn), rt.ptr(x_mid), rt.ptr(pred), rt.ptr(nz), rt.ptr(xin), float(c_skip),
                                        float(c_out), float(sigma_mid), float(dt_down), float(sigma_up), float(c_in_next),
                                        int(seed), int(step), int(sample0), B, C, L, Cp, 0, rt.ptr(ds), rt.current_stream()))
    return xn, xin


@adpm2_next.register_fake
def _(x, x_mid, pred, noise, c_skip, c_out, sigma_mid, dt_down, sigma_up, c_in_next, seed, step, sample0, dynamic_threshold=0.0):
    return x.new_empty(x.shape, dtype=torch.float32), pred.new_empty(pred.shape, dtype=torch.float32)


@custom_op("mdt::adpm2_euler", mutates_args=())
def adpm2_euler(x_base: Tensor, x_from: Tensor, denoised: Tensor, noise: Optional[Tensor], sigma: float, dt: float,
                sigma_up: float) -> Tensor:
    dev = _hip(x_base, x_from, denoised, noise)
    lib = rt.load_library()
    xb, xf, dn = _f32c(x_base), _f32c(x_from), _f32c(denoised)
    nz = None if noise is None else _f32c(noise)
    B, C, L = xb.shape
    out = torch.empty_like(xb)
    if B:
        with torch.cuda.device(dev):
            rt.check(lib.mdt_adpm2_euler(rt.ptr(xb), rt.ptr(xf), rt.ptr(dn), rt.ptr(nz), rt.ptr(out), float(sigma), float(dt),
                                         float(sigma_up), 0 if nz is None else 1, 0, 0, 0, B, C, L, rt.current_stream()))
    return out


@adpm2_euler.register_fake
def _(x_base, x_from, denoised, noise, sigma, dt, sigma_up):
    return x_base.new_empty(x_base.shape, dtype=torch.float32)


@custom_op("mdt::aeuler_next", mutates_args=())
def aeuler_next(x: Tensor, pred: Tensor, noise: Optional[Tensor], c_skip: float, c_out: float, sigma: float, dt: float,
                sigma_up: float, c_in_next: float, seed: int, step: int, sample0: int,
                dynamic_threshold: float = 0.0) -> Tuple[Tensor, Tensor]:
    """The whole AEulerSampler.step after its evaluation.  Returns (x_next, xin_next); noise None = counter-based generator."""
    dev = _hip(x, pred, noise)
    lib = rt.load_library()
    xn, pred = _f32c(x).clone(), _f32c(pred)
    nz = None if noise is None else _f32c(noise)
    B, C, L = xn.shape
    Cp = pred.shape[2]
    xin = torch.zeros(B, L, Cp, device=dev)
    if B:
        with torch.cuda.device(dev):
            ds = _dyn_scale(lib, xn, pred, c_skip, c_out, dynamic_threshold)
            rt.check(lib.mdt_aeuler_next(rt.ptr(xn), rt.ptr(pred), rt.ptr(nz), rt.ptr(xin), float(c_skip), float(c_out),
                                         float(sigma), float(dt), float(sigma_up), float(c_in_next), int(seed), int(step),
                                         int(sample0), B, C, L, Cp, 0, rt.ptr(ds), rt.current_stream()))
    return xn, xin


@aeuler_next.register_fake
def _(x, pred, noise, c_skip, c_out, sigma, dt, sigma_up, c_in_next, seed, step, sample0, dynamic_threshold=0.0):
    return x.new_empty(x.shape, dtype=torch.float32), pred.new_empty(pred.shape, dtype=torch.float32)


@custom_op("mdt::karras_hat", mutates_args=())
def karras_hat(x: Tensor, noise: Optional[Tensor], noise_scale: float, s_noise: float, c_in_hat: float, Cp: int, seed: int,
               step: int, sample0: int) -> Tuple[Tensor, Tensor]:
    """Churn stage of KarrasSampler.step.  Returns (x_hat, xin_hat)."""
    dev = _hip(x, noise)
    lib = rt.load_library()
    x = _f32c(x)
    nz = None if noise is None else _f32c(noise)
    B, C, L = x.shape
    if Cp < C or Cp % 16:
        raise RuntimeError(f"mdt::karras_hat: Cp={Cp} must be a multiple of 16 and >= C={C}")
    x_hat = torch.empty_like(x)
    xin = torch.zeros(B, L, Cp, device=dev)
    if B:
        with torch.cuda.device(dev):
            rt.check(lib.mdt_karras_hat(rt.ptr(x), rt.ptr(nz), rt.ptr(x_hat), rt.ptr(xin), float(noise_scale), float(s_noise),
                                        float(c_in_hat), int(seed), int(step), int(sample0), B, C, L, Cp, rt.current_stream()))
    return x_hat, xin


@karras_hat.register_fake
def _(x, noise, noise_scale, s_noise, c_in_hat, Cp, seed, step, sample0):
    return x.new_empty(x.shape, dtype=torch.float32), x.new_empty(x.shape[0], x.shape[2], Cp, dtype=torch.float32)


@custom_op("mdt::karras_mid", mutates_args=())
def karras_mid(x_hat: Tensor, pred: Tensor, c_skip: float, c_out: float, sigma_hat: float, dt: float, c_in_next: float,
               dynamic_threshold: float = 0.0) -> Tuple[Tensor, Tensor, Tensor]:
    """Euler move of KarrasSampler.step.  Returns (d, x_next, xin_next)."""
    dev = _hip(x_hat, pred)
    lib = rt.load_library()
    x_hat, pred = _f32c(x_hat), _f32c(pred)
    B, C, L = x_hat.shape
    Cp = pred.shape[2]
    d, x_next = torch.empty_like(x_hat), torch.empty_like(x_hat)
    xin = torch.zeros(B, L, Cp, device=dev)
    if B:
        with torch.cuda.device(dev):
            ds = _dyn_scale(lib, x_hat, pred, c_skip, c_out, dynamic_threshold)
            rt.check(lib.mdt_karras_mid(rt.ptr(x_hat), rt.ptr(pred), rt.ptr(d), rt.ptr(x_next), rt.ptr(xin), float(c_skip),
                                        float(c_out), float(sigma_hat), float(dt), float(c_in_next), B, C, L, Cp, 0, rt.ptr(ds),
                                        rt.current_stream()))
    return d, x_next, xin


@karras_mid.register_fake
def _(x_hat, pred, c_skip, c_out, sigma_hat, dt, c_in_next, dynamic_threshold=0.0):
    e = x_hat.new_empty(x_hat.shape, dtype=torch.float32)
    return e, x_hat.new_empty(x_hat.shape, dtype=torch.float32), pred.new_empty(pred.shape, dtype=torch.float32)


@custom_op("mdt::karras_next", mutates_args=())
def karras_next(x_hat: Tensor, x_next: Tensor, d: Tensor, pred: Tensor, c_skip: float, c_out: float, sigma_next: float,
                half: float, dynamic_threshold: float = 0.0) -> Tensor:
    """Correction of KarrasSampler.step as the reference writes it: x_hat + half * (d + d')."""
    dev = _hip(x_hat, x_next, d, pred)
    lib = rt.load_library()
    x_hat, x_next, d, pred = _f32c(x_hat), _f32c(x_next), _f32c(d), _f32c(pred)
    B, C, L = x_hat.shape
    out = torch.empty_like(x_hat)
    if B:
        with torch.cuda.device(dev):
            ds = _dyn_scale(lib, x_next, pred, c_skip, c_out, dynamic_threshold)
            rt.check(lib.mdt_karras_next(rt.ptr(x_hat), rt.ptr(x_next), rt.ptr(d), rt.ptr(pred), rt.ptr(out), float(c_skip),
                                         float(c_out), float(sigma_next), float(half), B, C, L, pred.shape[2], 0, rt.ptr(ds),
                                         rt.current_stream()))
    return out


@karras_next.register_fake
def _(x_hat, x_next, d, pred, c_skip, c_out, sigma_next, half, dynamic_threshold=0.0):
    return x_hat.new_empty(x_hat.shape, dtype=torch.float32)


@custom_op("mdt::argmax_tokens", mutates_args=())
def argmax_tokens(x: Tensor) -> Tensor:
    dev = _hip(x)
    lib = rt.load_library()
    x = _f32c(x)
    B, C, L = x.shape
    tok = torch.zeros(B, L, dtype=torch.int32, device=dev)
    if B:
        with torch.cuda.device(dev):
            rt.check(lib.mdt_argmax_tokens(rt.ptr(x), rt.ptr(tok), B, C, L, rt.current_stream()))
    return tok


@argmax_tokens.register_fake
def _(x):
    return x.new_empty(x.shape[0], x.shape[2], dtype=torch.int32)


# ----------------------------------------------------------------------------------------------------------------------
# candidate screening (csrc/k_screen.hip): rows are r = c * G + g, candidate c of group g
def _i32c(t: Tensor, what: str) -> Tensor:
    if t.dtype in (torch.bool,) or t.is_floating_point() or t.is_complex():
        raise RuntimeError(f"{what} must hold integers, got {t.dtype}")
    return t.detach().to(torch.int32).contiguous()


@custom_op("mdt::tokens_compact", mutates_args=())
def tokens_compact(tokens: Tensor, forward_length: int, x_norm: float) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """(B, L) ids -> (packed int32 (B, L), length int32 (B), key int64 (B): the bits of the uint64 key, forward input fp32
    (B, forward_length)); forward_length == 0: no forward input is written and (B, 0) is returned."""
    dev = _hip(tokens)
    lib = rt.load_library()
    if tokens.dim() != 2:
        raise RuntimeError("mdt::tokens_compact: tokens must be (B, L)")
    tok = _i32c(tokens, "mdt::tokens_compact: tokens")
    B, L = tok.shape
    if forward_length < 0:
        raise RuntimeError("mdt::tokens_compact: forward_length must not be negative")
    packed = torch.empty(B, L, dtype=torch.int32, device=dev)
    length = torch.empty(B, dtype=torch.int32, device=dev)
    key = torch.empty(B, dtype=torch.int64, device=dev)
    fwd = torch.empty(B, forward_length, dtype=torch.float32, device=dev)
    if B:
        with torch.cuda.device(dev):
            rt.check(lib.mdt_tokens_compact(rt.ptr(tok), B, L, rt.ptr(fwd) if forward_length else 0, forward_length, float(x_norm),
                                            rt.ptr(packed), rt.ptr(length), rt.ptr(key), rt.current_stream()))
    return packed, length, key, fwd


@tokens_compact.register_fake
def _(tokens, forward_length, x_norm):
    B, L = tokens.shape
    return (tokens.new_empty(B, L, dtype=torch.int32), tokens.new_empty(B, dtype=torch.int32),
            tokens.new_empty(B, dtype=torch.int64), tokens.new_empty(B, forward_length, dtype=torch.float32))


@custom_op("mdt::screen_score", mutates_args=())
def screen_score(props: Tensor, target: Tensor, weights: Optional[Tensor], candidates: int) -> Tensor:
    """props (N * G, ...) fp32, read in place: the first n values of every row; target (G, n); weights (n) or None -> (N * G)."""
    dev = _hip(props, target, weights)
    lib = rt.load_library()
    if target.dim() != 2:
        raise RuntimeError("mdt::screen_score: target must be (G, n)")
    G, n = target.shape
    rows = candidates * G
    if props.dim() < 2 or props.shape[0] != rows:
        raise RuntimeError(f"mdt::screen_score: props must hold candidates * G = {rows} rows")
    p, t = _f32c(props), _f32c(target)
    w = None if weights is None else _f32c(weights)
    if w is not None and tuple(w.shape) != (n,):
        raise RuntimeError("mdt::screen_score: weights must be (n,)")
    score = torch.empty(rows, dtype=torch.float32, device=dev)
    if rows:
        with torch.cuda.device(dev):
            rt.check(lib.mdt_screen_score(rt.ptr(p), p.numel() // rows, rt.ptr(t), rt.ptr(w), candidates, G, n, rt.ptr(score),
                                          rt.current_stream()))
    return score


@screen_score.register_fake
def _(props, target, weights, candidates):
    return props.new_empty(candidates * target.shape[0], dtype=torch.float32)


def _screen_select(op, score, key, packed, length, candidates, keep, known_key, known_packed, known_len, *, diverse=None,
                   reject=None, similar=None, classes=None):
    """The one body of the six selection ops: the argument checks, the three outputs, the call.  diverse: (known_dist, min_novelty,
    min_distance) of the ops that take them -- their rows have at most the 64 positions of the edit distance; reject: the byte per
    row, or None; similar: (fp, fp_count, sim_num) of mdt::screen_select_similar; classes: (class_key, max_per_class) of
    mdt::screen_select_classes.  The C symbol is the op's own, except that a
    ..._reject op whose reject is None calls the symbol without it: that op's launch, bit for bit."""
    known_dist, min_novelty, min_distance = diverse if diverse is not None else (None, 0, 0)
    fp, fp_count, sim_num = similar if similar is not None else (None, None, 0)
    class_key, max_per_class = classes if classes is not None else (None, 0)
    dev = _hip(score, key, packed, length, known_key, known_packed, known_len, known_dist, reject, fp, fp_count, class_key)
    lib = rt.load_library()
    rows, L = packed.shape
    N = candidates
    if N < 1 or rows % N:
        raise RuntimeError(f"{op}: {rows} rows are no multiple of candidates = {N}")
    G = rows // N
    if key.dtype != torch.int64 or packed.dtype != torch.int32 or length.dtype != torch.int32:
        raise RuntimeError(f"{op}: key must be int64, packed and length int32 (as mdt::tokens_compact returns them)")
    if score.numel() != rows or key.numel() != rows or length.numel() != rows:
        raise RuntimeError(f"{op}: score, key and length must hold one value per row of packed")
    known = (known_key, known_packed, known_len)
    if any(k is None for k in known) != all(k is None for k in known):
        raise RuntimeError(f"{op}: give known_key, known_packed and known_len together")
    M = 0
    if known_key is not None:
        M = known_key.numel()
        if known_key.dtype != torch.int64 or known_packed.dtype != torch.int32 or known_len.dtype != torch.int32:
            raise RuntimeError(f"{op}: known_key must be int64, known_packed and known_len int32")
        if tuple(known_packed.shape) != (M, L) or known_len.numel() != M:
            raise RuntimeError(f"{op}: the known set must be (M, {L}) rows with M keys and M lengths")
        known = tuple(k.contiguous() for k in known)
    if diverse is not None:
        if L > rt.EDIT_MAX_LENGTH:
            takes = "the edit distance takes" if similar is None else "the edit distance and the fingerprint take"
            raise RuntimeError(f"{op}: rows of {L} positions exceed the {rt.EDIT_MAX_LENGTH} {takes}")
        if known_dist is not None and (known_dist.dtype != torch.int32 or known_dist.numel() != rows):
            raise RuntimeError(f"{op}: known_dist must hold one int32 per row of packed")
        known_dist = None if known_dist is None else known_dist.contiguous()
    if (fp is None) != (fp_count is None):
        raise RuntimeError(f"{op}: fp and fp_count come together")
    if fp is not None:
        fp = _fp_rows(op, fp, "fp")
        if fp.shape[0] != rows or fp_count.dtype != torch.int32 or fp_count.numel() != rows:
            raise RuntimeError(f"{op}: fp and fp_count must hold one fingerprint and one int32 per row of packed")
        fp_count = fp_count.contiguous()
        if not 1 <= sim_num <= rt.FP_SIM_DEN:
            raise RuntimeError(f"{op}: sim_num = {sim_num} must lie in [1, {rt.FP_SIM_DEN}]")
    if class_key is not None:
        if class_key.dtype != torch.int64 or class_key.numel() != rows:
            raise RuntimeError(f"{op}: class_key must hold one int64 (the uint64 bits, as mdt::mol_key returns them) per row of packed")
        if max_per_class < 1:
            raise RuntimeError(f"{op}: max_per_class = {max_per_class} must be at least 1")
        class_key = class_key.contiguous()
    if reject is not None:
        if reject.dtype != torch.uint8 or reject.numel() != rows:
            raise RuntimeError(f"{op}: reject must hold one uint8 per row of packed")
        reject = reject.contiguous()
    score, key, packed, length = _f32c(score), key.contiguous(), packed.contiguous(), length.contiguous()
    status = torch.zeros(rows, dtype=torch.uint8, device=dev)
    index = torch.full((G, keep), -1, dtype=torch.int32, device=dev)
    count = torch.zeros(G, dtype=torch.int32, device=dev)
    if G:
        symbol = "mdt_" + op[len("mdt::"):]
        args = [rt.ptr(score), rt.ptr(key), rt.ptr(packed), rt.ptr(length), L, N, G, *(rt.ptr(k) if M else 0 for k in known), M, keep]
        if diverse is not None:
            args += [rt.ptr(known_dist), int(min_novelty), int(min_distance)]
        if similar is not None:
            args += [rt.ptr(reject), rt.ptr(fp), rt.ptr(fp_count), int(sim_num)]
            if classes is not None:
                args += [rt.ptr(class_key), int(max_per_class)]
        elif reject is not None:
            args += [rt.ptr(reject)]
        else:
            symbol = symbol.removesuffix("_reject")
        with torch.cuda.device(dev):
            rt.check(getattr(lib, symbol)(*args, rt.ptr(status), rt.ptr(index), rt.ptr(count), rt.current_stream()))
    return status, index, count


def _screen_select_fake(score, key, packed, length, candidates, keep, *optional):
    G = packed.shape[0] // candidates
    return (packed.new_empty(packed.shape[0], dtype=torch.uint8), packed.new_empty(G, keep, dtype=torch.int32),
            packed.new_empty(G, dtype=torch.int32))


@custom_op("mdt::screen_select", mutates_args=())
def screen_select(score: Tensor, key: Tensor, packed: Tensor, length: Tensor, candidates: int, keep: int,
                  known_key: Optional[Tensor], known_packed: Optional[Tensor],
                  known_len: Optional[Tensor]) -> Tuple[Tensor, Tensor, Tensor]:
    """-> (status uint8 (N * G), index int32 (G, K), count int32 (G)).  The known set: keys int64 (the uint64 bits, ascending AS
    uint64), packed rows int32 (M, L), lengths int32 (M) -- all three or none."""
    return _screen_select("mdt::screen_select", score, key, packed, length, candidates, keep, known_key, known_packed, known_len)


@custom_op("mdt::screen_select_diverse", mutates_args=())
def screen_select_diverse(score: Tensor, key: Tensor, packed: Tensor, length: Tensor, candidates: int, keep: int,
                          known_key: Optional[Tensor], known_packed: Optional[Tensor], known_len: Optional[Tensor],
                          known_dist: Optional[Tensor], min_novelty: int, min_distance: int) -> Tuple[Tensor, Tensor, Tensor]:
    """mdt::screen_select with the two edit-distance filters of mdt_screen_select_diverse (include/mdt_hip.h): bit 8 also where
    known_dist (int32 (N * G), or None) < min_novelty; the K best in (score, c) order that lie >= min_distance edits apart; bit 16
    on what a kept candidate pushed out.  Rows of at most 64 positions."""
    return _screen_select("mdt::screen_select_diverse", score, key, packed, length, candidates, keep, known_key, known_packed,
                          known_len, diverse=(known_dist, min_novelty, min_distance))


@custom_op("mdt::screen_select_reject", mutates_args=())
def screen_select_reject(score: Tensor, key: Tensor, packed: Tensor, length: Tensor, candidates: int, keep: int,
                         known_key: Optional[Tensor], known_packed: Optional[Tensor], known_len: Optional[Tensor],
                         reject: Optional[Tensor]) -> Tuple[Tensor, Tensor, Tensor]:
    """mdt::screen_select with ``reject`` (uint8 (N * G), e.g. mdt::smiles_check's status, or None): its bits are OR-ed into the
    status before eligibility is decided.  None: mdt::screen_select's launch, bit for bit."""
    return _screen_select("mdt::screen_select_reject", score, key, packed, length, candidates, keep, known_key, known_packed,
                          known_len, reject=reject)


@custom_op("mdt::screen_select_diverse_reject", mutates_args=())
def screen_select_diverse_reject(score: Tensor, key: Tensor, packed: Tensor, length: Tensor, candidates: int, keep: int,
                                 known_key: Optional[Tensor], known_packed: Optional[Tensor], known_len: Optional[Tensor],
                                 known_dist: Optional[Tensor], min_novelty: int, min_distance: int,
                                 reject: Optional[Tensor]) -> Tuple[Tensor, Tensor, Tensor]:
    """mdt::screen_select_diverse with ``reject`` as mdt::screen_select_reject takes it: a rejected candidate is not eligible, so
    it is never kept and never pushes another out under min_distance.  None: mdt::screen_select_diverse's launch, bit for bit."""
    return _screen_select("mdt::screen_select_diverse_reject", score, key, packed, length, candidates, keep, known_key, known_packed,
                          known_len, diverse=(known_dist, min_novelty, min_distance), reject=reject)


@custom_op("mdt::screen_select_similar", mutates_args=())
def screen_select_similar(score: Tensor, key: Tensor, packed: Tensor, length: Tensor, candidates: int, keep: int,
                          known_key: Optional[Tensor], known_packed: Optional[Tensor], known_len: Optional[Tensor],
                          known_dist: Optional[Tensor], min_novelty: int, min_distance: int, reject: Optional[Tensor],
                          fp: Optional[Tensor], fp_count: Optional[Tensor], sim_num: int) -> Tuple[Tensor, Tensor, Tensor]:
    """mdt::screen_select_diverse_reject with similarity as a second way to be passed over (mdt_screen_select_similar,
    include/mdt_hip.h): a candidate whose fingerprint (``fp`` int64 (N * G, 16), ``fp_count`` int32 (N * G), as mdt::mol_fp returns
    them) is at least sim_num / 65536 Tanimoto-similar to a candidate kept before it gets bit 16, as one closer than min_distance
    edits does.  fp and fp_count None: mdt::screen_select_diverse_reject's kernel on the same inputs, bit for bit."""
    return _screen_select("mdt::screen_select_similar", score, key, packed, length, candidates, keep, known_key, known_packed,
                          known_len, diverse=(known_dist, min_novelty, min_distance), reject=reject, similar=(fp, fp_count, sim_num))


@custom_op("mdt::screen_select_classes", mutates_args=())
def screen_select_classes(score: Tensor, key: Tensor, packed: Tensor, length: Tensor, candidates: int, keep: int,
                          known_key: Optional[Tensor], known_packed: Optional[Tensor], known_len: Optional[Tensor],
                          known_dist: Optional[Tensor], min_novelty: int, min_distance: int, reject: Optional[Tensor],
                          fp: Optional[Tensor], fp_count: Optional[Tensor], sim_num: int, class_key: Optional[Tensor],
                          max_per_class: int) -> Tuple[Tensor, Tensor, Tensor]:
    """mdt::screen_select_similar with classes as a third way to be passed over (mdt_screen_select_classes, include/mdt_hip.h): a
    candidate whose ``class_key`` (int64 (N * G): the uint64 bits, e.g. mdt::mol_key of the arrays of mdt::mol_scaffold) is not 0
    gets bit 16 when at least ``max_per_class`` candidates kept before it carry the same one; class 0 is never counted.  fp and
    fp_count may be None (no similarity test).  class_key None: mdt::screen_select_similar's launch on the same inputs, bit for
    bit."""
    return _screen_select("mdt::screen_select_classes", score, key, packed, length, candidates, keep, known_key, known_packed,
                          known_len, diverse=(known_dist, min_novelty, min_distance), reject=reject, similar=(fp, fp_count, sim_num),
                          classes=(class_key, max_per_class))


for _op in (screen_select, screen_select_diverse, screen_select_reject, screen_select_diverse_reject, screen_select_similar,
            screen_select_classes):
    _op.register_fake(_screen_select_fake)

# ----------------------------------------------------------------------------------------------------------------------
# well-formedness and valence of compacted id rows (csrc/k_smiles.hip): at most 128 positions, ids in [0, 256)
@custom_op("mdt::smiles_check", mutates_args=())
def smiles_check(packed: Tensor, length: Tensor, classes: Tensor, max_valence: Tensor, elements: Tensor) -> Tuple[Tensor, Tensor]:
    """-> (status uint8 (R,): 0 | 32 malformed | 64 overvalent, position int32 (R,): -1 for an OK row).  packed int32 (R, L) and
    length int32 (R) as mdt::tokens_compact returns them; classes uint8 (256), max_valence uint8 (10), elements int32 (26): the
    tables of mdt_smiles_check (include/mdt_hip.h), which SmilesVocabulary builds."""
    dev = _hip(packed, length, classes, max_valence, elements)
    lib = rt.load_library()
    op = "mdt::smiles_check"
    if packed.dim() != 2 or packed.dtype != torch.int32 or length.dtype != torch.int32 or length.numel() != packed.shape[0]:
        raise RuntimeError(f"{op}: packed must be int32 rows (R, L) with one int32 length each (as mdt::tokens_compact returns them)")
    R, L = packed.shape
    if not 1 <= L <= rt.SMILES_MAX_LENGTH:
        raise RuntimeError(f"{op}: packed has {L} positions per row, the check takes 1 to {rt.SMILES_MAX_LENGTH}")
    if classes.dtype != torch.uint8 or tuple(classes.shape) != (256,):
        raise RuntimeError(f"{op}: classes must be uint8 (256,)")
    if max_valence.dtype != torch.uint8 or tuple(max_valence.shape) != (10,):
        raise RuntimeError(f"{op}: max_valence must be uint8 (10,): B C N O P S F Cl Br I")
    if elements.dtype != torch.int32 or tuple(elements.shape) != (26,):
        raise RuntimeError(f"{op}: elements must be int32 (26,): one mask per uppercase letter")
    packed, length = packed.contiguous(), length.contiguous()
    classes, max_valence, elements = classes.contiguous(), max_valence.contiguous(), elements.contiguous()
    status = torch.zeros(R, dtype=torch.uint8, device=dev)
    position = torch.full((R,), -1, dtype=torch.int32, device=dev)
    if R:
        with torch.cuda.device(dev):
            rt.check(lib.mdt_smiles_check(rt.ptr(packed), rt.ptr(length), L, R, rt.ptr(classes), rt.ptr(max_valence),
                                          rt.ptr(elements), rt.ptr(status), rt.ptr(position), rt.current_stream()))
    return status, position


@smiles_check.register_fake
def _(packed, length, classes, max_valence, elements):
    R = packed.shape[0]
    return packed.new_empty(R, dtype=torch.uint8), packed.new_empty(R, dtype=torch.int32)


# ----------------------------------------------------------------------------------------------------------------------
# graph identity of compacted id rows (csrc/k_molgraph.hip): at most 64 positions, ids in [0, 256)
@custom_op("mdt::mol_graph", mutates_args=())
def mol_graph(packed: Tensor, length: Tensor, classes: Tensor, max_valence: Tensor,
              elements: Tensor) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """-> (natoms int32 (R,), atoms int32 (R, L): the uint32 descriptors' bits, nbonds int32 (R,), bonds int32 (R, L):
    a | b << 8 | order << 16, status uint8 (R,), position int32 (R,)): the molecular graph of every row that passes
    mdt::smiles_check's rules (status and position are that op's), as mdt_mol_graph defines it (include/mdt_hip.h).  Rows of status
    != 0 and empty rows have no atoms; words beyond the counts are 0.  Arguments as mdt::smiles_check, rows of at most 64 positions."""
    dev = _hip(packed, length, classes, max_valence, elements)
    lib = rt.load_library()
    op = "mdt::mol_graph"
    if packed.dim() != 2 or packed.dtype != torch.int32 or length.dtype != torch.int32 or length.numel() != packed.shape[0]:
        raise RuntimeError(f"{op}: packed must be int32 rows (R, L) with one int32 length each (as mdt::tokens_compact returns them)")
    R, L = packed.shape
    if not 1 <= L <= rt.MOL_MAX_LENGTH:
        raise RuntimeError(f"{op}: packed has {L} positions per row, the graph takes 1 to {rt.MOL_MAX_LENGTH}")
    if classes.dtype != torch.uint8 or tuple(classes.shape) != (256,):
        raise RuntimeError(f"{op}: classes must be uint8 (256,)")
    if max_valence.dtype != torch.uint8 or tuple(max_valence.shape) != (10,):
        raise RuntimeError(f"{op}: max_valence must be uint8 (10,): B C N O P S F Cl Br I")
    if elements.dtype != torch.int32 or tuple(elements.shape) != (26,):
        raise RuntimeError(f"{op}: elements must be int32 (26,): one mask per uppercase letter")
    packed, length = packed.contiguous(), length.contiguous()
    classes, max_valence, elements = classes.contiguous(), max_valence.contiguous(), elements.contiguous()
    natoms = torch.zeros(R, dtype=torch.int32, device=dev)
    atoms = torch.zeros(R, L, dtype=torch.int32, device=dev)
    nbonds = torch.zeros(R, dtype=torch.int32, device=dev)
    bonds = torch.zeros(R, L, dtype=torch.int32, device=dev)
    status = torch.zeros(R, dtype=torch.uint8, device=dev)
    position = torch.full((R,), -1, dtype=torch.int32, device=dev)
    if R:
        with torch.cuda.device(dev):
            rt.check(lib.mdt_mol_graph(rt.ptr(packed), rt.ptr(length), L, R, rt.ptr(classes), rt.ptr(max_valence), rt.ptr(elements),
                                       rt.ptr(natoms), rt.ptr(atoms), rt.ptr(nbonds), rt.ptr(bonds), rt.ptr(status),
                                       rt.ptr(position), rt.current_stream()))
    return natoms, atoms, nbonds, bonds, status, position


@mol_graph.register_fake
def _(packed, length, classes, max_valence, elements):
    R, L = packed.shape
    return (packed.new_empty(R, dtype=torch.int32), packed.new_empty(R, L, dtype=torch.int32),
            packed.new_empty(R, dtype=torch.int32), packed.new_empty(R, L, dtype=torch.int32),
            packed.new_empty(R, dtype=torch.uint8), packed.new_empty(R, dtype=torch.int32))


@custom_op("mdt::mol_key", mutates_args=())
def mol_key(natoms: Tensor, atoms: Tensor, nbonds: Tensor, bonds: Tensor) -> Tensor:
    """-> key int64 (R,): the uint64 bits of mdt_mol_key's graph key (include/mdt_hip.h) for the graph arrays of mdt::mol_graph;
    0 where natoms is 0 (no molecule)."""
    dev = _hip(natoms, atoms, nbonds, bonds)
    lib = rt.load_library()
    op = "mdt::mol_key"
    if atoms.dim() != 2 or tuple(bonds.shape) != tuple(atoms.shape) or any(t.dtype != torch.int32 for t in (natoms, atoms, nbonds, bonds)):
        raise RuntimeError(f"{op}: atoms and bonds must be int32 (R, L), natoms and nbonds int32 (as mdt::mol_graph returns them)")
    R, L = atoms.shape
    if natoms.numel() != R or nbonds.numel() != R:
        raise RuntimeError(f"{op}: natoms and nbonds must hold one value per row of atoms")
    if not 1 <= L <= rt.MOL_MAX_LENGTH:
        raise RuntimeError(f"{op}: atoms has {L} positions per row, the key takes 1 to {rt.MOL_MAX_LENGTH}")
    natoms, atoms, nbonds, bonds = natoms.contiguous(), atoms.contiguous(), nbonds.contiguous(), bonds.contiguous()
    key = torch.zeros(R, dtype=torch.int64, device=dev)
    if R:
        with torch.cuda.device(dev):
            rt.check(lib.mdt_mol_key(rt.ptr(natoms), rt.ptr(atoms), rt.ptr(nbonds), rt.ptr(bonds), L, R, rt.ptr(key),
                                     rt.current_stream()))
    return key


@mol_key.register_fake
def _(natoms, atoms, nbonds, bonds):
    return atoms.new_empty(atoms.shape[0], dtype=torch.int64)


@custom_op("mdt::key_flags", mutates_args=())
def key_flags(key: Tensor, candidates: int, known_key: Optional[Tensor]) -> Tensor:
    """-> flags uint8 (N * G,), row c * G + g: 4 (duplicate) where a candidate c' < c of the same group has the same non-zero key,
    8 (known) where the non-zero key is in ``known_key`` (int64 (M,): uint64 bits ASCENDING as unsigned, or None).  Key 0: neither."""
    dev = _hip(key, known_key)
    lib = rt.load_library()
    op = "mdt::key_flags"
    N = candidates
    if key.dim() != 1 or key.dtype != torch.int64:
        raise RuntimeError(f"{op}: key must be int64 (N * G,)")
    rows = key.numel()
    if not 1 <= N <= rt.MAX_KEY_CANDIDATES or rows % N:
        raise RuntimeError(f"{op}: candidates = {N} must lie in [1, {rt.MAX_KEY_CANDIDATES}] and divide the {rows} rows")
    M = 0
    if known_key is not None:
        if known_key.dim() != 1 or known_key.dtype != torch.int64:
            raise RuntimeError(f"{op}: known_key must be int64 (M,)")
        M, known_key = known_key.numel(), known_key.contiguous()
    key = key.contiguous()
    flags = torch.zeros(rows, dtype=torch.uint8, device=dev)
    if rows:
        with torch.cuda.device(dev):
            rt.check(lib.mdt_key_flags(rt.ptr(key), N, rows // N, rt.ptr(known_key) if M else 0, M, rt.ptr(flags), rt.current_stream()))
    return flags


@key_flags.register_fake
def _(key, candidates, known_key):
    return key.new_empty(key.shape[0], dtype=torch.uint8)


# ----------------------------------------------------------------------------------------------------------------------
# Tanimoto similarity on graph fingerprints (csrc/k_molfp.hip): 1024 bits as 16 int64 words (the uint64 bits) per row
def _fp_rows(op, fp, what):
    if fp.dim() != 2 or fp.dtype != torch.int64 or fp.shape[1] != rt.FP_WORDS:
        raise RuntimeError(f"{op}: {what} must be int64 (R, {rt.FP_WORDS}): the uint64 words of mdt::mol_fp")
    return fp.contiguous()


@custom_op("mdt::mol_fp", mutates_args=())
def mol_fp(natoms: Tensor, atoms: Tensor, nbonds: Tensor, bonds: Tensor, radius: int) -> Tuple[Tensor, Tensor]:
    """-> (fp int64 (R, 16): the uint64 bits of mdt_mol_fp's 1024-bit circular fingerprint (include/mdt_hip.h) for the graph arrays
    of mdt::mol_graph, count int32 (R,): its set bits); all zero where natoms is 0 (no molecule).  0 <= radius <= 3.  Not RDKit's
    Morgan / ECFP."""
    dev = _hip(natoms, atoms, nbonds, bonds)
    lib = rt.load_library()
    op = "mdt::mol_fp"
    if atoms.dim() != 2 or tuple(bonds.shape) != tuple(atoms.shape) or any(t.dtype != torch.int32 for t in (natoms, atoms, nbonds, bonds)):
        raise RuntimeError(f"{op}: atoms and bonds must be int32 (R, L), natoms and nbonds int32 (as mdt::mol_graph returns them)")
    R, L = atoms.shape
    if natoms.numel() != R or nbonds.numel() != R:
        raise RuntimeError(f"{op}: natoms and nbonds must hold one value per row of atoms")
    if not 1 <= L <= rt.MOL_MAX_LENGTH:
        raise RuntimeError(f"{op}: atoms has {L} positions per row, the fingerprint takes 1 to {rt.MOL_MAX_LENGTH}")
    if not 0 <= radius <= rt.FP_MAX_RADIUS:
        raise RuntimeError(f"{op}: radius = {radius} must lie in [0, {rt.FP_MAX_RADIUS}]")
    natoms, atoms, nbonds, bonds = natoms.contiguous(), atoms.contiguous(), nbonds.contiguous(), bonds.contiguous()
    fp = torch.zeros(R, rt.FP_WORDS, dtype=torch.int64, device=dev)
    count = torch.zeros(R, dtype=torch.int32, device=dev)
    if R:
        with torch.cuda.device(dev):
            rt.check(lib.mdt_mol_fp(rt.ptr(natoms), rt.ptr(atoms), rt.ptr(nbonds), rt.ptr(bonds), L, R, int(radius), rt.ptr(fp),
                                    rt.ptr(count), rt.current_stream()))
    return fp, count


@mol_fp.register_fake
def _(natoms, atoms, nbonds, bonds, radius):
    R = atoms.shape[0]
    return atoms.new_empty(R, rt.FP_WORDS, dtype=torch.int64), atoms.new_empty(R, dtype=torch.int32)


@custom_op("mdt::fp_tanimoto", mutates_args=())
def fp_tanimoto(a_fp: Tensor, b_fp: Tensor) -> Tuple[Tensor, Tensor]:
    """-> (inter int32 (R,), union int32 (R,)): popcount(A & B) and |A| + |B| - inter of row r of a against row r of b; the Tanimoto
    similarity is inter / union, 0 where union is 0."""
    dev = _hip(a_fp, b_fp)
    lib = rt.load_library()
    a, b = _fp_rows("mdt::fp_tanimoto", a_fp, "a_fp"), _fp_rows("mdt::fp_tanimoto", b_fp, "b_fp")
    if a.shape != b.shape:
        raise RuntimeError(f"mdt::fp_tanimoto: a_fp {tuple(a.shape)} and b_fp {tuple(b.shape)} must have the same shape")
    R = a.shape[0]
    inter = torch.zeros(R, dtype=torch.int32, device=dev)
    union = torch.zeros(R, dtype=torch.int32, device=dev)
    if R:
        with torch.cuda.device(dev):
            rt.check(lib.mdt_fp_tanimoto_rows(rt.ptr(a), rt.ptr(b), R, rt.ptr(inter), rt.ptr(union), rt.current_stream()))
    return inter, union


@fp_tanimoto.register_fake
def _(a_fp, b_fp):
    R = a_fp.shape[0]
    return a_fp.new_empty(R, dtype=torch.int32), a_fp.new_empty(R, dtype=torch.int32)


@custom_op("mdt::fp_nearest", mutates_args=())
def fp_nearest(fp: Tensor, known_fp: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """-> (index int32 (R,), inter int32 (R,), union int32 (R,)): per row the LOWEST row of ``known_fp`` (M >= 1 fingerprints) that
    attains the largest Tanimoto similarity to it, and the counts of that pair.  Exact, and independent of how the work is split."""
    dev = _hip(fp, known_fp)
    lib = rt.load_library()
    q, k = _fp_rows("mdt::fp_nearest", fp, "fp"), _fp_rows("mdt::fp_nearest", known_fp, "known_fp")
    if k.shape[0] < 1:
        raise RuntimeError("mdt::fp_nearest: the known set is empty (need M >= 1)")
    R = q.shape[0]
    index = torch.zeros(R, dtype=torch.int32, device=dev)
    inter = torch.zeros(R, dtype=torch.int32, device=dev)
    union = torch.zeros(R, dtype=torch.int32, device=dev)
    best = torch.empty(R, dtype=torch.int64, device=dev)            # the packed maxima (quotient << 32 | ~index), one word per row
    if R:
        with torch.cuda.device(dev):
            rt.check(lib.mdt_fp_nearest(rt.ptr(q), R, rt.ptr(k), k.shape[0], rt.ptr(best), rt.ptr(inter), rt.ptr(union),
                                        rt.ptr(index), rt.current_stream()))
    return index, inter, union


@fp_nearest.register_fake
def _(fp, known_fp):
    R = fp.shape[0]
    return tuple(fp.new_empty(R, dtype=torch.int32) for _ in range(3))


# ----------------------------------------------------------------------------------------------------------------------
# graph substructure match (csrc/k_molsub.hip): up to 32 patterns of up to 32 positions against rows of up to 64
@custom_op("mdt::sub_match", mutates_args=())
def sub_match(natoms: Tensor, atoms: Tensor, nbonds: Tensor, bonds: Tensor, p_natoms: Tensor, p_atoms: Tensor, p_nbonds: Tensor,
              p_bonds: Tensor, need: int, ban: int) -> Tuple[Tensor, Tensor, Tensor]:
    """-> (match int32 (R,), undecided int32 (R,): the uint32 bits, bit q = the verdict for pattern q of mdt_sub_match
    (include/mdt_hip.h) on the graph arrays of mdt::mol_graph -- targets (R, L <= 64), patterns (P <= 32, LP <= 32); flags uint8
    (R,): 128 where a pattern of the mask ``need`` is not matched or one of ``ban`` is matched or undecided).  Subgraph
    monomorphism under a step cap; not SMARTS, not RDKit's HasSubstructMatch."""
    dev = _hip(natoms, atoms, nbonds, bonds, p_natoms, p_atoms, p_nbonds, p_bonds)
    lib = rt.load_library()
    op = "mdt::sub_match"
    for what, n_, a_, nb_, b_ in (("", natoms, atoms, nbonds, bonds), ("p_", p_natoms, p_atoms, p_nbonds, p_bonds)):
        if a_.dim() != 2 or tuple(b_.shape) != tuple(a_.shape) or any(t.dtype != torch.int32 for t in (n_, a_, nb_, b_)):
            raise RuntimeError(f"{op}: {what}atoms and {what}bonds must be int32 (rows, width), {what}natoms and {what}nbonds int32 "
                               "(as mdt::mol_graph returns them)")
        if n_.numel() != a_.shape[0] or nb_.numel() != a_.shape[0]:
            raise RuntimeError(f"{op}: {what}natoms and {what}nbonds must hold one value per row of {what}atoms")
    (R, L), (P, LP) = atoms.shape, p_atoms.shape
    if not 1 <= L <= rt.MOL_MAX_LENGTH:
        raise RuntimeError(f"{op}: atoms has {L} positions per row, the match takes 1 to {rt.MOL_MAX_LENGTH}")
    if not 1 <= LP <= rt.SUB_MAX_WIDTH:
        raise RuntimeError(f"{op}: p_atoms has {LP} positions per pattern, the match takes 1 to {rt.SUB_MAX_WIDTH}")
    if not 1 <= P <= rt.SUB_MAX_PATTERNS:
        raise RuntimeError(f"{op}: {P} patterns, the match takes 1 to {rt.SUB_MAX_PATTERNS} a call")
    if not (0 <= need < 1 << P and 0 <= ban < 1 << P):
        raise RuntimeError(f"{op}: need = {need:#x} and ban = {ban:#x} may only have bits below P = {P}")
    if need & ban:
        raise RuntimeError(f"{op}: need = {need:#x} and ban = {ban:#x} overlap")
    natoms, atoms, nbonds, bonds = natoms.contiguous(), atoms.contiguous(), nbonds.contiguous(), bonds.contiguous()
    p_natoms, p_atoms, p_nbonds, p_bonds = p_natoms.contiguous(), p_atoms.contiguous(), p_nbonds.contiguous(), p_bonds.contiguous()
    match = torch.zeros(R, dtype=torch.int32, device=dev)
    undecided = torch.zeros(R, dtype=torch.int32, device=dev)
    flags = torch.zeros(R, dtype=torch.uint8, device=dev)
    if R:
        with torch.cuda.device(dev):
            rt.check(lib.mdt_sub_match(rt.ptr(natoms), rt.ptr(atoms), rt.ptr(nbonds), rt.ptr(bonds), L, R, rt.ptr(p_natoms),
                                       rt.ptr(p_atoms), rt.ptr(p_nbonds), rt.ptr(p_bonds), LP, P, int(need), int(ban),
                                       rt.ptr(match), rt.ptr(undecided), rt.ptr(flags), rt.current_stream()))
    return match, undecided, flags


@sub_match.register_fake
def _(natoms, atoms, nbonds, bonds, p_natoms, p_atoms, p_nbonds, p_bonds, need, ban):
    R = atoms.shape[0]
    return (atoms.new_empty(R, dtype=torch.int32), atoms.new_empty(R, dtype=torch.int32), atoms.new_empty(R, dtype=torch.uint8))


@custom_op("mdt::sub_map", mutates_args=())
def sub_map(natoms: Tensor, atoms: Tensor, nbonds: Tensor, bonds: Tensor, p_natoms: Tensor, p_atoms: Tensor, p_nbonds: Tensor,
            p_bonds: Tensor, count_lo: Optional[Tensor], count_hi: Optional[Tensor]) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """-> (found int64 (R, P), capped int64 (R, P): the uint64 bits, bit t = root t saw an embedding / was abandoned; embeddings
    int32 (R, P); cover int64 (R, P): the uint64 bits, the target atoms in some embedding seen; map uint8 (R, P, LP): 1 + f(p) of
    the first map of the lowest found root; flags uint8 (R,)) of mdt_sub_map (include/mdt_hip.h) on the graph arrays of
    mdt::mol_graph -- targets (R, L <= 64), patterns (P <= 32, LP <= 32).  ``count_lo`` / ``count_hi``: uint8 (P,), both or neither;
    with them flags is 128 where the number of anchors of some pattern lies outside its bounds (abandoned roots count against the
    row both ways), without them all zero.  The enumeration of mdt::sub_match's search under its step cap; anchors, not atom sets;
    not SMARTS, not RDKit's GetSubstructMatches."""
    dev = _hip(natoms, atoms, nbonds, bonds, p_natoms, p_atoms, p_nbonds, p_bonds)
    lib = rt.load_library()
    op = "mdt::sub_map"
    for what, n_, a_, nb_, b_ in (("", natoms, atoms, nbonds, bonds), ("p_", p_natoms, p_atoms, p_nbonds, p_bonds)):
        if a_.dim() != 2 or tuple(b_.shape) != tuple(a_.shape) or any(t.dtype != torch.int32 for t in (n_, a_, nb_, b_)):
            raise RuntimeError(f"{op}: {what}atoms and {what}bonds must be int32 (rows, width), {what}natoms and {what}nbonds int32 "
                               "(as mdt::mol_graph returns them)")
        if n_.numel() != a_.shape[0] or nb_.numel() != a_.shape[0]:
            raise RuntimeError(f"{op}: {what}natoms and {what}nbonds must hold one value per row of {what}atoms")
    (R, L), (P, LP) = atoms.shape, p_atoms.shape
    if not 1 <= L <= rt.MOL_MAX_LENGTH:
        raise RuntimeError(f"{op}: atoms has {L} positions per row, the match takes 1 to {rt.MOL_MAX_LENGTH}")
    if not 1 <= LP <= rt.SUB_MAX_WIDTH:
        raise RuntimeError(f"{op}: p_atoms has {LP} positions per pattern, the match takes 1 to {rt.SUB_MAX_WIDTH}")
    if not 1 <= P <= rt.SUB_MAX_PATTERNS:
        raise RuntimeError(f"{op}: {P} patterns, the match takes 1 to {rt.SUB_MAX_PATTERNS} a call")
    if (count_lo is None) != (count_hi is None):
        raise RuntimeError(f"{op}: count_lo and count_hi must be given together or not at all")
    for name, t in (("count_lo", count_lo), ("count_hi", count_hi)):
        if t is not None and (t.dtype != torch.uint8 or tuple(t.shape) != (P,)):
            raise RuntimeError(f"{op}: {name} must be uint8 with one bound per pattern, ({P},)")
    natoms, atoms, nbonds, bonds = natoms.contiguous(), atoms.contiguous(), nbonds.contiguous(), bonds.contiguous()
    p_natoms, p_atoms, p_nbonds, p_bonds = p_natoms.contiguous(), p_atoms.contiguous(), p_nbonds.contiguous(), p_bonds.contiguous()
    found = torch.zeros(R, P, dtype=torch.int64, device=dev)
    capped = torch.zeros(R, P, dtype=torch.int64, device=dev)
    embeddings = torch.zeros(R, P, dtype=torch.int32, device=dev)
    cover = torch.zeros(R, P, dtype=torch.int64, device=dev)
    fmap = torch.zeros(R, P, LP, dtype=torch.uint8, device=dev)
    flags = torch.zeros(R, dtype=torch.uint8, device=dev)
    if R:
        bounds = (None, None, None) if count_lo is None else (count_lo.contiguous(), count_hi.contiguous(), flags)
        with torch.cuda.device(dev):
            rt.check(lib.mdt_sub_map(rt.ptr(natoms), rt.ptr(atoms), rt.ptr(nbonds), rt.ptr(bonds), L, R, rt.ptr(p_natoms),
                                     rt.ptr(p_atoms), rt.ptr(p_nbonds), rt.ptr(p_bonds), LP, P, rt.ptr(bounds[0]), rt.ptr(bounds[1]),
                                     rt.ptr(found), rt.ptr(capped), rt.ptr(embeddings), rt.ptr(cover), rt.ptr(fmap),
                                     rt.ptr(bounds[2]), rt.current_stream()))
    return found, capped, embeddings, cover, fmap, flags


@sub_map.register_fake
def _(natoms, atoms, nbonds, bonds, p_natoms, p_atoms, p_nbonds, p_bonds, count_lo, count_hi):
    (R, L), (P, LP) = atoms.shape, p_atoms.shape
    return (atoms.new_empty((R, P), dtype=torch.int64), atoms.new_empty((R, P), dtype=torch.int64),
            atoms.new_empty((R, P), dtype=torch.int32), atoms.new_empty((R, P), dtype=torch.int64),
            atoms.new_empty((R, P, LP), dtype=torch.uint8), atoms.new_empty(R, dtype=torch.uint8))


# ----------------------------------------------------------------------------------------------------------------------
# maximum common substructure of row pairs (csrc/k_molmcs.hip): rows of at most 64 positions on either side
@custom_op("mdt::mol_mcs", mutates_args=())
def mol_mcs(a_natoms: Tensor, a_atoms: Tensor, a_nbonds: Tensor, a_bonds: Tensor, b_natoms: Tensor, b_atoms: Tensor, b_nbonds: Tensor,
            b_bonds: Tensor, mode: int) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """-> (size int32 (R, 2): bonds, atoms; map_a uint8 (R, LA): 1 + the partner of each A atom; bond_a int64 (R,): the uint64 bits,
    bit e = A entry e is matched; steps int32 (R,); natoms int32 (R,), atoms int32 (R, LA), nbonds int32 (R,), bonds int32 (R, LA),
    atom_map uint8 (R, LA): the common substructure as graph arrays in mdt::mol_scaffold's format; flags uint8 (R,): 1 a pair of
    molecules, 2 something in common, 4 undecided (a root was capped: a lower bound), 8 all of A, 16 all of B) of mdt_mol_mcs
    (include/mdt_hip.h) on the graph arrays of mdt::mol_graph or mdt::mol_normalize -- A (R, LA <= 64) against B (R or 1, LB <= 64).
    mode bit 0 (runtime.MCS_EXACT_ATOMS): whole atom words must be equal, not only symbol and aromatic bit.  The greatest CONNECTED
    common subgraph by (bonds, atoms), edge kind, under a step cap per root; not RDKit's FindMCS."""
    dev = _hip(a_natoms, a_atoms, a_nbonds, a_bonds, b_natoms, b_atoms, b_nbonds, b_bonds)
    lib = rt.load_library()
    op = "mdt::mol_mcs"
    for what, n_, a_, nb_, b_ in (("a_", a_natoms, a_atoms, a_nbonds, a_bonds), ("b_", b_natoms, b_atoms, b_nbonds, b_bonds)):
        if a_.dim() != 2 or tuple(b_.shape) != tuple(a_.shape) or any(t.dtype != torch.int32 for t in (n_, a_, nb_, b_)):
            raise RuntimeError(f"{op}: {what}atoms and {what}bonds must be int32 (rows, width), {what}natoms and {what}nbonds int32 "
                               "(as mdt::mol_graph returns them)")
        if n_.numel() != a_.shape[0] or nb_.numel() != a_.shape[0]:
            raise RuntimeError(f"{op}: {what}natoms and {what}nbonds must hold one value per row of {what}atoms")
        if not 1 <= a_.shape[1] <= rt.MOL_MAX_LENGTH:
            raise RuntimeError(f"{op}: {what}atoms has {a_.shape[1]} positions per row, the search takes 1 to {rt.MOL_MAX_LENGTH}")
    (R, LA), (RB, LB) = a_atoms.shape, b_atoms.shape
    if RB != R and RB != 1:
        raise RuntimeError(f"{op}: b has {RB} rows; it takes {R} (row by row) or 1 (every a row against the one b row)")
    if mode & ~rt.MCS_EXACT_ATOMS:
        raise RuntimeError(f"{op}: mode = {mode} must be 0 or MCS_EXACT_ATOMS (1)")
    a_natoms, a_atoms, a_nbonds, a_bonds = (t.contiguous() for t in (a_natoms, a_atoms, a_nbonds, a_bonds))
    b_natoms, b_atoms, b_nbonds, b_bonds = (t.contiguous() for t in (b_natoms, b_atoms, b_nbonds, b_bonds))
    size = torch.zeros(R, 2, dtype=torch.int32, device=dev)
    map_a = torch.zeros(R, LA, dtype=torch.uint8, device=dev)
    bond_a = torch.zeros(R, dtype=torch.int64, device=dev)
    steps = torch.zeros(R, dtype=torch.int32, device=dev)
    out_natoms = torch.zeros(R, dtype=torch.int32, device=dev)
    out_atoms = torch.zeros(R, LA, dtype=torch.int32, device=dev)
    out_nbonds = torch.zeros(R, dtype=torch.int32, device=dev)
    out_bonds = torch.zeros(R, LA, dtype=torch.int32, device=dev)
    atom_map = torch.zeros(R, LA, dtype=torch.uint8, device=dev)
    flags = torch.zeros(R, dtype=torch.uint8, device=dev)
    if R:
        with torch.cuda.device(dev):
            rt.check(lib.mdt_mol_mcs(rt.ptr(a_natoms), rt.ptr(a_atoms), rt.ptr(a_nbonds), rt.ptr(a_bonds), LA, R, rt.ptr(b_natoms),
                                     rt.ptr(b_atoms), rt.ptr(b_nbonds), rt.ptr(b_bonds), LB, RB, int(mode), rt.ptr(size),
                                     rt.ptr(map_a), rt.ptr(bond_a), rt.ptr(steps), rt.ptr(out_natoms), rt.ptr(out_atoms),
                                     rt.ptr(out_nbonds), rt.ptr(out_bonds), rt.ptr(atom_map), rt.ptr(flags), rt.current_stream()))
    return size, map_a, bond_a, steps, out_natoms, out_atoms, out_nbonds, out_bonds, atom_map, flags


@mol_mcs.register_fake
def _(a_natoms, a_atoms, a_nbonds, a_bonds, b_natoms, b_atoms, b_nbonds, b_bonds, mode):
    R, LA = a_atoms.shape
    return (a_atoms.new_empty((R, 2), dtype=torch.int32), a_atoms.new_empty((R, LA), dtype=torch.uint8),
            a_atoms.new_empty(R, dtype=torch.int64), a_atoms.new_empty(R, dtype=torch.int32), a_atoms.new_empty(R, dtype=torch.int32),
            a_atoms.new_empty((R, LA), dtype=torch.int32), a_atoms.new_empty(R, dtype=torch.int32),
            a_atoms.new_empty((R, LA), dtype=torch.int32), a_atoms.new_empty((R, LA), dtype=torch.uint8),
            a_atoms.new_empty(R, dtype=torch.uint8))


# ----------------------------------------------------------------------------------------------------------------------
# implicit hydrogens, the Kekule check and the formula (csrc/k_molh.hip): rows of at most 64 positions
@custom_op("mdt::mol_hydrogens", mutates_args=())
def mol_hydrogens(natoms: Tensor, atoms: Tensor, nbonds: Tensor, bonds: Tensor, max_steps: int) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """-> (hydrogens uint8 (R, L), partner uint8 (R, L), verdict uint8 (R,), atom int32 (R,), formula int32 (R, 13)) of
    mdt_mol_hydrogens (include/mdt_hip.h) for the graph arrays of mdt::mol_graph: per atom the hydrogens it carries and, where the
    verdict is 0, 1 + the atom its double bond goes to (0: none); verdict 0 ok, 1 an aromatic atom is overvalent (``atom``), 2 no
    Kekule structure, 3 undecided after ``max_steps`` (1..4096) tries; formula: H B C N O F P S Cl Br I other charge.  All zero
    (atom -1) where natoms is 0 (no molecule).  Not RDKit's sanitisation."""
    dev = _hip(natoms, atoms, nbonds, bonds)
    lib = rt.load_library()
    op = "mdt::mol_hydrogens"
    if atoms.dim() != 2 or tuple(bonds.shape) != tuple(atoms.shape) or any(t.dtype != torch.int32 for t in (natoms, atoms, nbonds, bonds)):
        raise RuntimeError(f"{op}: atoms and bonds must be int32 (R, L), natoms and nbonds int32 (as mdt::mol_graph returns them)")
    R, L = atoms.shape
    if natoms.numel() != R or nbonds.numel() != R:
        raise RuntimeError(f"{op}: natoms and nbonds must hold one value per row of atoms")
    if not 1 <= L <= rt.MOL_MAX_LENGTH:
        raise RuntimeError(f"{op}: atoms has {L} positions per row, the hydrogens take 1 to {rt.MOL_MAX_LENGTH}")
    if not 1 <= max_steps <= rt.MOLH_MAX_STEPS:
        raise RuntimeError(f"{op}: max_steps = {max_steps} must lie in [1, {rt.MOLH_MAX_STEPS}]")
    natoms, atoms, nbonds, bonds = natoms.contiguous(), atoms.contiguous(), nbonds.contiguous(), bonds.contiguous()
    hydrogens = torch.zeros(R, L, dtype=torch.uint8, device=dev)
    partner = torch.zeros(R, L, dtype=torch.uint8, device=dev)
    verdict = torch.zeros(R, dtype=torch.uint8, device=dev)
    atom = torch.full((R,), -1, dtype=torch.int32, device=dev)
    formula = torch.zeros(R, rt.MOLH_FORMULA, dtype=torch.int32, device=dev)
    if R:
        with torch.cuda.device(dev):
            rt.check(lib.mdt_mol_hydrogens(rt.ptr(natoms), rt.ptr(atoms), rt.ptr(nbonds), rt.ptr(bonds), L, R, int(max_steps),
                                           rt.ptr(hydrogens), rt.ptr(partner), rt.ptr(verdict), rt.ptr(atom), rt.ptr(formula),
                                           rt.current_stream()))
    return hydrogens, partner, verdict, atom, formula


@mol_hydrogens.register_fake
def _(natoms, atoms, nbonds, bonds, max_steps):
    R, L = atoms.shape
    return (atoms.new_empty(R, L, dtype=torch.uint8), atoms.new_empty(R, L, dtype=torch.uint8), atoms.new_empty(R, dtype=torch.uint8),
            atoms.new_empty(R, dtype=torch.int32), atoms.new_empty(R, rt.MOLH_FORMULA, dtype=torch.int32))


# ----------------------------------------------------------------------------------------------------------------------
# ring perception and descriptors (csrc/k_molring.hip): rows of at most 64 positions
@custom_op("mdt::mol_rings", mutates_args=())
def mol_rings(natoms: Tensor, atoms: Tensor, nbonds: Tensor, bonds: Tensor, hydrogens: Tensor, lo: Optional[Tensor],
              hi: Optional[Tensor]) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """-> (bond_ring uint8 (R, L), atom_ring uint8 (R, L), descriptors int32 (R, 16), flags uint8 (R,)) of mdt_mol_rings
    (include/mdt_hip.h) for the graph arrays of mdt::mol_graph and the hydrogens of mdt::mol_hydrogens: per bond entry and per atom
    the size of the smallest cycle through it (0: none), per row the sixteen descriptors (enum mdt_molr_slot), and 128 where
    ``lo`` / ``hi`` (int32 (16,), both or neither) are given and a descriptor of a molecule row lies outside them.  All zero where
    natoms is 0 (no molecule).  Not RDKit's ring info, not an SSSR."""
    dev = _hip(natoms, atoms, nbonds, bonds, hydrogens, lo, hi)
    lib = rt.load_library()
    op = "mdt::mol_rings"
    if atoms.dim() != 2 or tuple(bonds.shape) != tuple(atoms.shape) or any(t.dtype != torch.int32 for t in (natoms, atoms, nbonds, bonds)):
        raise RuntimeError(f"{op}: atoms and bonds must be int32 (R, L), natoms and nbonds int32 (as mdt::mol_graph returns them)")
    R, L = atoms.shape
    if natoms.numel() != R or nbonds.numel() != R:
        raise RuntimeError(f"{op}: natoms and nbonds must hold one value per row of atoms")
    if not 1 <= L <= rt.MOL_MAX_LENGTH:
        raise RuntimeError(f"{op}: atoms has {L} positions per row, the rings take 1 to {rt.MOL_MAX_LENGTH}")
    if hydrogens.dtype != torch.uint8 or tuple(hydrogens.shape) != (R, L):
        raise RuntimeError(f"{op}: hydrogens must be uint8 ({R}, {L}) (as mdt::mol_hydrogens returns them)")
    if (lo is None) != (hi is None):
        raise RuntimeError(f"{op}: lo and hi are given together or not at all")
    for name, t in (("lo", lo), ("hi", hi)):
        if t is not None and (t.dtype != torch.int32 or tuple(t.shape) != (rt.MOLR_DESC,)):
            raise RuntimeError(f"{op}: {name} must be int32 ({rt.MOLR_DESC},)")
    natoms, atoms, nbonds, bonds, hydrogens = (t.contiguous() for t in (natoms, atoms, nbonds, bonds, hydrogens))
    lo, hi = (None, None) if lo is None else (lo.contiguous(), hi.contiguous())
    bond_ring = torch.zeros(R, L, dtype=torch.uint8, device=dev)
    atom_ring = torch.zeros(R, L, dtype=torch.uint8, device=dev)
    desc = torch.zeros(R, rt.MOLR_DESC, dtype=torch.int32, device=dev)
    flags = torch.zeros(R, dtype=torch.uint8, device=dev)
    if R:
        with torch.cuda.device(dev):
            rt.check(lib.mdt_mol_rings(rt.ptr(natoms), rt.ptr(atoms), rt.ptr(nbonds), rt.ptr(bonds), rt.ptr(hydrogens), L, R,
                                       rt.ptr(lo), rt.ptr(hi), rt.ptr(bond_ring), rt.ptr(atom_ring), rt.ptr(desc), rt.ptr(flags),
                                       rt.current_stream()))
    return bond_ring, atom_ring, desc, flags


@mol_rings.register_fake
def _(natoms, atoms, nbonds, bonds, hydrogens, lo, hi):
    R, L = atoms.shape
    return (atoms.new_empty(R, L, dtype=torch.uint8), atoms.new_empty(R, L, dtype=torch.uint8),
            atoms.new_empty(R, rt.MOLR_DESC, dtype=torch.int32), atoms.new_empty(R, dtype=torch.uint8))


# ----------------------------------------------------------------------------------------------------------------------
# the normal form of a graph row (csrc/k_molnorm.hip): rows of at most 64 positions
@custom_op("mdt::mol_normalize", mutates_args=())
def mol_normalize(natoms: Tensor, atoms: Tensor, nbonds: Tensor, bonds: Tensor, hydrogens: Tensor, partner: Tensor, verdict: Tensor,
                  bond_ring: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """-> (atoms int32 (R, L), bonds int32 (R, L), flags uint8 (R,)) of mdt_mol_normalize (include/mdt_hip.h) for the graph arrays
    of mdt::mol_graph, the hydrogens, partner and verdict of mdt::mol_hydrogens and the bond_ring of mdt::mol_rings: graph arrays in
    the same format, indices preserved (natoms and nbonds are reused), in which the Kekule, the aromatic and the bracket spelling of
    a molecule are one; flags 1 normalised, 2 an aromatic ring, 4 something differs from what was written.  A row of verdict != 0
    comes back as written, a row that is no molecule all zero, both with flags 0.  Not RDKit's aromaticity model."""
    dev = _hip(natoms, atoms, nbonds, bonds, hydrogens, partner, verdict, bond_ring)
    lib = rt.load_library()
    op = "mdt::mol_normalize"
    if atoms.dim() != 2 or tuple(bonds.shape) != tuple(atoms.shape) or any(t.dtype != torch.int32 for t in (natoms, atoms, nbonds, bonds)):
        raise RuntimeError(f"{op}: atoms and bonds must be int32 (R, L), natoms and nbonds int32 (as mdt::mol_graph returns them)")
    R, L = atoms.shape
    if natoms.numel() != R or nbonds.numel() != R:
        raise RuntimeError(f"{op}: natoms and nbonds must hold one value per row of atoms")
    if not 1 <= L <= rt.MOL_MAX_LENGTH:
        raise RuntimeError(f"{op}: atoms has {L} positions per row, the normal form takes 1 to {rt.MOL_MAX_LENGTH}")
    for name, t in (("hydrogens", hydrogens), ("partner", partner)):
        if t.dtype != torch.uint8 or tuple(t.shape) != (R, L):
            raise RuntimeError(f"{op}: {name} must be uint8 ({R}, {L}) (as mdt::mol_hydrogens returns it)")
    if verdict.dtype != torch.uint8 or tuple(verdict.shape) != (R,):
        raise RuntimeError(f"{op}: verdict must be uint8 ({R},) (as mdt::mol_hydrogens returns it)")
    if bond_ring.dtype != torch.uint8 or tuple(bond_ring.shape) != (R, L):
        raise RuntimeError(f"{op}: bond_ring must be uint8 ({R}, {L}) (as mdt::mol_rings returns it)")
    natoms, atoms, nbonds, bonds, hydrogens, partner, verdict, bond_ring = (
        t.contiguous() for t in (natoms, atoms, nbonds, bonds, hydrogens, partner, verdict, bond_ring))
    out_atoms = torch.zeros(R, L, dtype=torch.int32, device=dev)
    out_bonds = torch.zeros(R, L, dtype=torch.int32, device=dev)
    flags = torch.zeros(R, dtype=torch.uint8, device=dev)
    if R:
        with torch.cuda.device(dev):
            rt.check(lib.mdt_mol_normalize(rt.ptr(natoms), rt.ptr(atoms), rt.ptr(nbonds), rt.ptr(bonds), rt.ptr(hydrogens),
                                           rt.ptr(partner), rt.ptr(verdict), rt.ptr(bond_ring), L, R, rt.ptr(out_atoms),
                                           rt.ptr(out_bonds), rt.ptr(flags), rt.current_stream()))
    return out_atoms, out_bonds, flags


@mol_normalize.register_fake
def _(natoms, atoms, nbonds, bonds, hydrogens, partner, verdict, bond_ring):
    R, L = atoms.shape
    return (atoms.new_empty(R, L, dtype=torch.int32), atoms.new_empty(R, L, dtype=torch.int32), atoms.new_empty(R, dtype=torch.uint8))


# ----------------------------------------------------------------------------------------------------------------------
# the scaffold of a graph row (csrc/k_molscaf.hip): rows of at most 64 positions
@custom_op("mdt::mol_scaffold", mutates_args=())
def mol_scaffold(natoms: Tensor, atoms: Tensor, nbonds: Tensor, bonds: Tensor,
                 mode: int) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """-> (natoms int32 (R,), atoms int32 (R, L), nbonds int32 (R,), bonds int32 (R, L), atom_map uint8 (R, L), flags uint8 (R,)) of
    mdt_mol_scaffold (include/mdt_hip.h) for the graph arrays of mdt::mol_graph or of mdt::mol_normalize: the 2-core of the ring
    graph -- rings plus linkers -- with mode bit 0 (runtime.MOLS_EXOCYCLIC) plus the atoms double-bonded to it, renumbered, as graph
    arrays that mdt::mol_key takes; mode bit 1 (runtime.MOLS_GENERIC) makes every atom a plain C and every bond single.  atom_map:
    1 + the new index of a kept atom, else 0; flags 1 a molecule, 2 it has a scaffold, 4 nothing was pruned.  An acyclic molecule
    has no scaffold: all zero.  Not RDKit's MurckoScaffold."""
    dev = _hip(natoms, atoms, nbonds, bonds)
    lib = rt.load_library()
    op = "mdt::mol_scaffold"
    if atoms.dim() != 2 or tuple(bonds.shape) != tuple(atoms.shape) or any(t.dtype != torch.int32 for t in (natoms, atoms, nbonds, bonds)):
        raise RuntimeError(f"{op}: atoms and bonds must be int32 (R, L), natoms and nbonds int32 (as mdt::mol_graph returns them)")
    R, L = atoms.shape
    if natoms.numel() != R or nbonds.numel() != R:
        raise RuntimeError(f"{op}: natoms and nbonds must hold one value per row of atoms")
    if not 1 <= L <= rt.MOL_MAX_LENGTH:
        raise RuntimeError(f"{op}: atoms has {L} positions per row, the scaffold takes 1 to {rt.MOL_MAX_LENGTH}")
    if not 0 <= mode <= (rt.MOLS_EXOCYCLIC | rt.MOLS_GENERIC):
        raise RuntimeError(f"{op}: mode = {mode} must be 0 or a sum of MOLS_EXOCYCLIC (1) and MOLS_GENERIC (2)")
    natoms, atoms, nbonds, bonds = (t.contiguous() for t in (natoms, atoms, nbonds, bonds))
    out_natoms = torch.zeros(R, dtype=torch.int32, device=dev)
    out_atoms = torch.zeros(R, L, dtype=torch.int32, device=dev)
    out_nbonds = torch.zeros(R, dtype=torch.int32, device=dev)
    out_bonds = torch.zeros(R, L, dtype=torch.int32, device=dev)
    atom_map = torch.zeros(R, L, dtype=torch.uint8, device=dev)
    flags = torch.zeros(R, dtype=torch.uint8, device=dev)
    if R:
        with torch.cuda.device(dev):
            rt.check(lib.mdt_mol_scaffold(rt.ptr(natoms), rt.ptr(atoms), rt.ptr(nbonds), rt.ptr(bonds), L, R, int(mode),
                                          rt.ptr(out_natoms), rt.ptr(out_atoms), rt.ptr(out_nbonds), rt.ptr(out_bonds),
                                          rt.ptr(atom_map), rt.ptr(flags), rt.current_stream()))
    return out_natoms, out_atoms, out_nbonds, out_bonds, atom_map, flags


@mol_scaffold.register_fake
def _(natoms, atoms, nbonds, bonds, mode):
    R, L = atoms.shape
    return (atoms.new_empty(R, dtype=torch.int32), atoms.new_empty(R, L, dtype=torch.int32), atoms.new_empty(R, dtype=torch.int32),
            atoms.new_empty(R, L, dtype=torch.int32), atoms.new_empty(R, L, dtype=torch.uint8), atoms.new_empty(R, dtype=torch.uint8))


# ----------------------------------------------------------------------------------------------------------------------
# graph rows back to token rows (csrc/k_molwrite.hip): rows of at most 64 positions, written rows of at most 128 tokens
def _graph_arrays(op, natoms, atoms, nbonds, bonds, what):
    if atoms.dim() != 2 or tuple(bonds.shape) != tuple(atoms.shape) or any(t.dtype != torch.int32 for t in (natoms, atoms, nbonds, bonds)):
        raise RuntimeError(f"{op}: atoms and bonds must be int32 (R, L), natoms and nbonds int32 (as mdt::mol_graph returns them)")
    R, L = atoms.shape
    if natoms.numel() != R or nbonds.numel() != R:
        raise RuntimeError(f"{op}: natoms and nbonds must hold one value per row of atoms")
    if not 1 <= L <= rt.MOL_MAX_LENGTH:
        raise RuntimeError(f"{op}: atoms has {L} positions per row, {what} takes 1 to {rt.MOL_MAX_LENGTH}")
    return R, L


@custom_op("mdt::mol_rank", mutates_args=())
def mol_rank(natoms: Tensor, atoms: Tensor, nbonds: Tensor, bonds: Tensor) -> Tensor:
    """-> priority int64 (R, L): the uint64 bits of mdt_mol_rank (include/mdt_hip.h) for graph arrays in mdt::mol_graph's format --
    per atom the label it has in mdt::mol_key's refinement under the root of its component whose rooted hash is the smallest (ties:
    the lowest index): a visiting priority that does not depend on the numbering.  0 beyond natoms and for a row that is no
    molecule."""
    dev = _hip(natoms, atoms, nbonds, bonds)
    lib = rt.load_library()
    op = "mdt::mol_rank"
    R, L = _graph_arrays(op, natoms, atoms, nbonds, bonds, "the priority")
    natoms, atoms, nbonds, bonds = (t.contiguous() for t in (natoms, atoms, nbonds, bonds))
    priority = torch.zeros(R, L, dtype=torch.int64, device=dev)
    if R:
        with torch.cuda.device(dev):
            rt.check(lib.mdt_mol_rank(rt.ptr(natoms), rt.ptr(atoms), rt.ptr(nbonds), rt.ptr(bonds), L, R, rt.ptr(priority),
                                      rt.current_stream()))
    return priority


@mol_rank.register_fake
def _(natoms, atoms, nbonds, bonds):
    return atoms.new_empty(atoms.shape, dtype=torch.int64)


@custom_op("mdt::mol_canon", mutates_args=())
def mol_canon(natoms: Tensor, atoms: Tensor, nbonds: Tensor, bonds: Tensor) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """-> (priority int64 (R, L), canon_atoms int32 (R, L), canon_bonds int32 (R, L), nodes int32 (R,), flags uint8 (R,)) of
    mdt_mol_canon (include/mdt_hip.h) for graph arrays in mdt::mol_graph's format: 1 + the canonical position of every atom (what
    mdt::mol_write takes as its priority), the row relabelled -- the atom words in canonical position and the entries lo | hi << 8 |
    order << 16 in ascending (lo, hi, order), zero beyond the counts -- the nodes of the search trees, and flags: 1 canonical; 2
    undecided, the search passed 4,096 nodes: the three arrays are all zero; 0 no molecule.  Two decided rows are the same
    molecular graph exactly when their counts and relabelled arrays are equal."""
    dev = _hip(natoms, atoms, nbonds, bonds)
    lib = rt.load_library()
    op = "mdt::mol_canon"
    R, L = _graph_arrays(op, natoms, atoms, nbonds, bonds, "the canonical order")
    natoms, atoms, nbonds, bonds = (t.contiguous() for t in (natoms, atoms, nbonds, bonds))
    priority = torch.empty(R, L, dtype=torch.int64, device=dev)           # (the kernel defines every word: no fill launches)
    canon_atoms = torch.empty(R, L, dtype=torch.int32, device=dev)
    canon_bonds = torch.empty(R, L, dtype=torch.int32, device=dev)
    nodes = torch.empty(R, dtype=torch.int32, device=dev)
    flags = torch.empty(R, dtype=torch.uint8, device=dev)
    if R:
        with torch.cuda.device(dev):
            rt.check(lib.mdt_mol_canon(rt.ptr(natoms), rt.ptr(atoms), rt.ptr(nbonds), rt.ptr(bonds), L, R, rt.ptr(priority),
                                       rt.ptr(canon_atoms), rt.ptr(canon_bonds), rt.ptr(nodes), rt.ptr(flags), rt.current_stream()))
    return priority, canon_atoms, canon_bonds, nodes, flags


@mol_canon.register_fake
def _(natoms, atoms, nbonds, bonds):
    R = atoms.shape[0]
    return (atoms.new_empty(atoms.shape, dtype=torch.int64), atoms.new_empty(atoms.shape, dtype=torch.int32),
            atoms.new_empty(atoms.shape, dtype=torch.int32), atoms.new_empty(R, dtype=torch.int32), atoms.new_empty(R, dtype=torch.uint8))


@custom_op("mdt::mol_write", mutates_args=())
def mol_write(natoms: Tensor, atoms: Tensor, nbonds: Tensor, bonds: Tensor, priority: Optional[Tensor], class_id: Tensor,
              width: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """-> (tokens int32 (R, W), length int32 (R,), token_atom uint8 (R, W), flags uint8 (R,)) of mdt_mol_write (include/mdt_hip.h):
    graph arrays in mdt::mol_graph's format spelled as SMILES token rows of ``width`` = W positions, zero after the ``length``
    tokens.  priority: int64 (R, L) as mdt::mol_rank returns it, or None: the atoms are visited as numbered.  class_id: uint8
    (128,), the token id of every class of mdt::smiles_check's class table, 0 for none.  token_atom: 1 + the atom a token belongs
    to, 0 for a dot.  flags: 1 written; 2 length > W; 4 the vocabulary lacks a class the row needs; 8 not writable (an entry
    (a, a), a pair named twice, an order outside 1..5, an atom word mdt::mol_graph cannot have written); with 2, 4 and 8 the tokens
    are all zero.  Not a canonical form and not RDKit's canonical SMILES."""
    dev = _hip(natoms, atoms, nbonds, bonds, priority, class_id)
    lib = rt.load_library()
    op = "mdt::mol_write"
    R, L = _graph_arrays(op, natoms, atoms, nbonds, bonds, "the writer")
    if not 1 <= width <= rt.MOLW_MAX_WIDTH:
        raise RuntimeError(f"{op}: width = {width}, the writer writes rows of 1 to {rt.MOLW_MAX_WIDTH} tokens")
    if priority is not None and (priority.dtype != torch.int64 or tuple(priority.shape) != (R, L)):
        raise RuntimeError(f"{op}: priority must be int64 (R, L) (as mdt::mol_rank returns it) or None")
    if class_id.dtype != torch.uint8 or tuple(class_id.shape) != (128,):
        raise RuntimeError(f"{op}: class_id must be uint8 (128,)")
    natoms, atoms, nbonds, bonds = (t.contiguous() for t in (natoms, atoms, nbonds, bonds))
    priority = None if priority is None else priority.contiguous()
    class_id = class_id.contiguous()
    W = int(width)
    tokens = torch.zeros(R, W, dtype=torch.int32, device=dev)
    length = torch.zeros(R, dtype=torch.int32, device=dev)
    token_atom = torch.zeros(R, W, dtype=torch.uint8, device=dev)
    flags = torch.zeros(R, dtype=torch.uint8, device=dev)
    if R:
        with torch.cuda.device(dev):
            rt.check(lib.mdt_mol_write(rt.ptr(natoms), rt.ptr(atoms), rt.ptr(nbonds), rt.ptr(bonds), rt.ptr(priority), L, R,
                                       rt.ptr(class_id), W, rt.ptr(tokens), rt.ptr(length), rt.ptr(token_atom), rt.ptr(flags),
                                       rt.current_stream()))
    return tokens, length, token_atom, flags


@mol_write.register_fake
def _(natoms, atoms, nbonds, bonds, priority, class_id, width):
    R = atoms.shape[0]
    return (atoms.new_empty(R, width, dtype=torch.int32), atoms.new_empty(R, dtype=torch.int32),
            atoms.new_empty(R, width, dtype=torch.uint8), atoms.new_empty(R, dtype=torch.uint8))


# ----------------------------------------------------------------------------------------------------------------------
# edit distance between compacted id rows (csrc/k_edit.hip): at most 64 positions, ids in [0, 64)
def _edit_rows(op, packed, length, what):
    if packed.dim() != 2 or packed.dtype != torch.int32 or length.dtype != torch.int32 or length.numel() != packed.shape[0]:
        raise RuntimeError(f"{op}: {what} must be int32 rows (R, L) with one int32 length each (as mdt::tokens_compact returns them)")
    if not 1 <= packed.shape[1] <= rt.EDIT_MAX_LENGTH:
        raise RuntimeError(f"{op}: {what} has {packed.shape[1]} positions per row, the edit distance takes 1 to {rt.EDIT_MAX_LENGTH}")
    return packed.contiguous(), length.contiguous()


@custom_op("mdt::edit_distance", mutates_args=())
def edit_distance(a_packed: Tensor, a_len: Tensor, b_packed: Tensor, b_len: Tensor) -> Tensor:
    """-> int32 (R,): the Levenshtein distance of row r of a to row r of b."""
    dev = _hip(a_packed, a_len, b_packed, b_len)
    lib = rt.load_library()
    a, al = _edit_rows("mdt::edit_distance", a_packed, a_len, "a")
    b, bl = _edit_rows("mdt::edit_distance", b_packed, b_len, "b")
    if a.shape != b.shape:
        raise RuntimeError(f"mdt::edit_distance: a {tuple(a.shape)} and b {tuple(b.shape)} must have the same shape")
    R, L = a.shape
    dist = torch.empty(R, dtype=torch.int32, device=dev)
    if R:
        with torch.cuda.device(dev):
            rt.check(lib.mdt_edit_distance_rows(rt.ptr(a), rt.ptr(al), rt.ptr(b), rt.ptr(bl), L, R, rt.ptr(dist), rt.current_stream()))
    return dist


@edit_distance.register_fake
def _(a_packed, a_len, b_packed, b_len):
    return a_packed.new_empty(a_packed.shape[0], dtype=torch.int32)


@custom_op("mdt::edit_nearest", mutates_args=())
def edit_nearest(packed: Tensor, length: Tensor, known_packed: Tensor, known_len: Tensor) -> Tuple[Tensor, Tensor]:
    """-> (distance int32 (R,), index int32 (R,)): per row the smallest distance to a row of the known set (M >= 1 rows of the
    same width) and the lowest known index that attains it."""
    dev = _hip(packed, length, known_packed, known_len)
    lib = rt.load_library()
    q, ql = _edit_rows("mdt::edit_nearest", packed, length, "packed")
    k, kl = _edit_rows("mdt::edit_nearest", known_packed, known_len, "known_packed")
    if k.shape[1] != q.shape[1]:
        raise RuntimeError(f"mdt::edit_nearest: the known rows have {k.shape[1]} positions, the query rows {q.shape[1]}")
    if k.shape[0] < 1:
        raise RuntimeError("mdt::edit_nearest: the known set is empty (need M >= 1)")
    R, L = q.shape
    dist = torch.empty(R, dtype=torch.int32, device=dev)
    index = torch.empty(R, dtype=torch.int32, device=dev)
    best = torch.empty(R, dtype=torch.int64, device=dev)            # the packed minima (distance << 32 | index), one word per row
    if R:
        with torch.cuda.device(dev):
            rt.check(lib.mdt_edit_nearest(rt.ptr(q), rt.ptr(ql), L, R, rt.ptr(k), rt.ptr(kl), k.shape[0], rt.ptr(best), rt.ptr(dist),
                                          rt.ptr(index), rt.current_stream()))
    return dist, index


@edit_nearest.register_fake
def _(packed, length, known_packed, known_len):
    R = packed.shape[0]
    return packed.new_empty(R, dtype=torch.int32), packed.new_empty(R, dtype=torch.int32)


# ----------------------------------------------------------------------------------------------------------------------
# the network and the whole loop: `handle` names the model's compiled engine (packed weights, programs, HIP graphs)
# ----------------------------------------------------------------------------------------------------------------------
@custom_op("mdt::unet_eval", mutates_args=())
def unet_eval(xin: Tensor, embedding: Tensor, c_noise: float, embedding_scale: float, handle: int) -> Tensor:
    """xin (B, L, Cp) token-major network input, embedding (B, n, F); returns the prediction (B, L, Cp)."""
    dev = _hip(xin, embedding)
    lib = rt.load_library()
    eng = _engine_on(handle, dev, "mdt::unet_eval")
    xin = _f32c(xin)
    B = xin.shape[0]
    if tuple(xin.shape[1:]) != (eng.c.length, eng.c.in_pad):
        raise RuntimeError(f"mdt::unet_eval: xin {tuple(xin.shape)} is not (B, {eng.c.length}, {eng.c.in_pad})")
    if B == 0:
        return torch.empty_like(xin)
    with torch.no_grad(), torch.cuda.device(dev):
        eng.reserve(B)
        eng.prepare_context(embedding)
        eng.prepare_times(torch.tensor([float(c_noise)]))
        eng.select_time(0)
        eng.xin.copy_(xin)
        eng.handoff_check()
        pred = eng.eval(False)
        if embedding_scale != 1.0:
            um = eng.eval(True)
            rt.check(lib.mdt_cfg_mix(rt.ptr(pred), rt.ptr(um), rt.ptr(pred), float(embedding_scale), pred.numel(),
                                     rt.current_stream()))
        out = pred.clone()
        eng.note_handoff()          # pair hand-off status: checked before the prediction is returned (engine.py)
        return out


@unet_eval.register_fake
def _(xin, embedding, c_noise, embedding_scale, handle):
    return xin.new_empty(xin.shape, dtype=torch.float32)


def _rows_engine(handle: int, dev, what: str):
    eng = _engine_on(handle, dev, what)
    if not eng.c.rows:
        raise RuntimeError(f"{what}: the handle names an engine of the shared-row programs; the per-row form is compiled with "
                           "compile_unet(rows=True) (model.engine(device, n_ctx, batch, rows=True))")
    return eng


def _eval_rows(lib, eng, embedding: Tensor, c_noise: Tensor, embedding_scale: float) -> Tensor:
    """eng.xin holds the network input of the reserved batch: context, per-sample time rows, one evaluation (two + the guidance
    mix for embedding_scale != 1) -> eng.pred."""
    eng.prepare_context(embedding)
    eng.prepare_time_rows(c_noise)
    eng.handoff_check()
    pred = eng.eval_rows(False)
    if embedding_scale != 1.0:
        um = eng.eval_rows(True)
        rt.check(lib.mdt_cfg_mix(rt.ptr(pred), rt.ptr(um), rt.ptr(pred), float(embedding_scale), pred.numel(), rt.current_stream()))
    return pred


@custom_op("mdt::precond_in_rows", mutates_args=())
def precond_in_rows(x: Tensor, c_in: Tensor, Cp: int) -> Tensor:
    """xin[b] = c_in[b] * x[b], token-major and padded (diffusion.py:810 with one sigma per sample)."""
    dev = _hip(x, c_in)
    lib = rt.load_library()
    x, c_in = _f32c(x), _f32c(c_in).flatten()
    B, C, L = x.shape
    if Cp < C or Cp % 16 or c_in.numel() != B:
        raise RuntimeError(f"mdt::precond_in_rows: Cp={Cp} must be a multiple of 16 and >= C={C}, c_in must hold B={B} values")
    out = torch.zeros(B, L, Cp, device=dev)
    if B:
        with torch.cuda.device(dev):
            rt.check(lib.mdt_precond_in_rows(rt.ptr(x), rt.ptr(out), rt.ptr(c_in), B, C, L, Cp, rt.current_stream()))
    return out


@precond_in_rows.register_fake
def _(x, c_in, Cp):
    return x.new_empty(x.shape[0], x.shape[2], Cp, dtype=torch.float32)


@custom_op("mdt::precond_out_rows", mutates_args=())
def precond_out_rows(x: Tensor, pred: Tensor, c_skip: Tensor, c_out: Tensor, dynamic_threshold: float = 0.0) -> Tensor:
    """D[b] = clip(c_skip[b] x[b] + c_out[b] pred[b], dynamic_threshold) (diffusion.py:811-814 with one sigma per sample)."""
    dev = _hip(x, pred, c_skip, c_out)
    lib = rt.load_library()
    x, pred, c_skip, c_out = _f32c(x), _f32c(pred), _f32c(c_skip).flatten(), _f32c(c_out).flatten()
    B, C, L = x.shape
    if pred.dim() != 3 or pred.shape[0] != B or pred.shape[1] != L or pred.shape[2] < C:
        raise RuntimeError(f"mdt::precond_out_rows: pred {tuple(pred.shape)} is not token-major (B, L, Cp) for x {tuple(x.shape)}")
    if c_skip.numel() != B or c_out.numel() != B:
        raise RuntimeError(f"mdt::precond_out_rows: c_skip / c_out must hold B={B} values")
    out = torch.empty_like(x)
    if B:
        with torch.cuda.device(dev):
            ds = None
            if dynamic_threshold:
                ds = torch.empty(B, device=dev)
                rt.check(lib.mdt_dyn_scale_rows(rt.ptr(x), rt.ptr(pred), rt.ptr(ds), rt.ptr(c_skip), rt.ptr(c_out),
                                                float(dynamic_threshold), B, C, L, pred.shape[2], rt.current_stream()))
            rt.check(lib.mdt_precond_out_rows(rt.ptr(x), rt.ptr(pred), rt.ptr(out), rt.ptr(c_skip), rt.ptr(c_out), B, C, L,
                                              pred.shape[2], rt.ptr(ds), rt.current_stream()))
    return out


@precond_out_rows.register_fake
def _(x, pred, c_skip, c_out, dynamic_threshold=0.0):
    return x.new_empty(x.shape, dtype=torch.float32)


@custom_op("mdt::unet_eval_rows", mutates_args=())
def unet_eval_rows(xin: Tensor, embedding: Tensor, c_noise: Tensor, embedding_scale: float, handle: int) -> Tensor:
    """mdt::unet_eval with one time value per sample: xin (B, L, Cp), embedding (B, n, F), c_noise (B,); ONE evaluation of the
    per-row program whatever the number of distinct values.  `handle` names an engine of the per-row form."""
    dev = _hip(xin, embedding, c_noise)
    lib = rt.load_library()
    eng = _rows_engine(handle, dev, "mdt::unet_eval_rows")
    xin = _f32c(xin)
    B = xin.shape[0]
    if tuple(xin.shape[1:]) != (eng.c.length, eng.c.in_pad):
        raise RuntimeError(f"mdt::unet_eval_rows: xin {tuple(xin.shape)} is not (B, {eng.c.length}, {eng.c.in_pad})")
    if c_noise.numel() != B:
        raise RuntimeError(f"mdt::unet_eval_rows: c_noise holds {c_noise.numel()} values for a batch of {B}")
    if B == 0:
        return torch.empty_like(xin)
    with torch.no_grad(), torch.cuda.device(dev):
        eng.reserve(B)
        eng.xin.copy_(xin)
        out = _eval_rows(lib, eng, embedding, c_noise, float(embedding_scale)).clone()
        eng.note_handoff()
        return out


@unet_eval_rows.register_fake
def _(xin, embedding, c_noise, embedding_scale, handle):
    return xin.new_empty(xin.shape, dtype=torch.float32)


@custom_op("mdt::eval_loss", mutates_args=())
def eval_loss(x0: Tensor, noise: Optional[Tensor], embedding: Tensor, coef: Tensor, handle: int, dynamic_threshold: float,
              seed: int, sample0: int) -> Tensor:
    """KDiffusion_mod.forward's per-sample weighted losses (diffusion.py:820-844) on the kernels: x0 (B, C, L) the clean target,
    noise (B, C, L) or None (counter-based generator keyed by (seed, sample0 + b)), embedding (B, n, F), coef (6, B) = sigma | c_in |
    c_skip | c_out | c_noise | loss_weight (diffusion.RowWeights.packed()).  Returns (B,) = loss_weight * mean((D - x0)^2)."""
    dev = _hip(x0, noise, embedding, coef)
    lib = rt.load_library()
    eng = _rows_engine(handle, dev, "mdt::eval_loss")
    x0, coef = _f32c(x0), _f32c(coef)
    nz = None if noise is None else _f32c(noise)
    B, C, L = x0.shape
    Cp = eng.c.in_pad
    if L != eng.c.length or C > Cp or tuple(coef.shape) != (6, B) or (nz is not None and nz.shape != x0.shape):
        raise RuntimeError(f"mdt::eval_loss: x0 {tuple(x0.shape)} / noise / coef {tuple(coef.shape)} do not fit (B, C <= {Cp}, "
                           f"{eng.c.length}) and (6, B)")
    loss = torch.empty(B, device=dev)
    if B == 0:
        return loss
    sigma, c_in, c_skip, c_out, c_noise, weight = (coef[k] for k in range(6))
    with torch.no_grad(), torch.cuda.device(dev):
        eng.reserve(B)
        x_noisy = torch.empty_like(x0)
        rt.check(lib.mdt_noise_in_rows(rt.ptr(x0), rt.ptr(nz), rt.ptr(sigma), rt.ptr(c_in), rt.ptr(x_noisy), rt.ptr(eng.xin),
                                       int(seed), 0, int(sample0), B, C, L, Cp, rt.current_stream()))
        pred = _eval_rows(lib, eng, embedding, c_noise, 1.0)
        ds = None
        if dynamic_threshold:
            ds = torch.empty(B, device=dev)
            rt.check(lib.mdt_dyn_scale_rows(rt.ptr(x_noisy), rt.ptr(pred), rt.ptr(ds), rt.ptr(c_skip), rt.ptr(c_out),
                                            float(dynamic_threshold), B, C, L, Cp, rt.current_stream()))
        rt.check(lib.mdt_loss_rows(rt.ptr(x0), rt.ptr(x_noisy), rt.ptr(pred), rt.ptr(c_skip), rt.ptr(c_out), rt.ptr(weight),
                                   rt.ptr(ds), rt.ptr(loss), B, C, L, Cp, rt.current_stream()))
        eng.note_handoff()
    return loss


@eval_loss.register_fake
def _(x0, noise, embedding, coef, handle, dynamic_threshold, seed, sample0):
    return x0.new_empty(x0.shape[0], dtype=torch.float32)


SAMPLER_KINDS = {kind: i for i, kind in enumerate(FUSED_SAMPLERS)}      # sampler_kind of mdt::sample_with


def sampler_spec(sampler) -> Tuple[int, list]:
    """(sampler_kind, sampler_params) of mdt::sample_with for a sampler object that may take the fused loop."""
    kind = require_fused_kind(sampler)
    return SAMPLER_KINDS[kind], [float(getattr(sampler, name)) for name in FUSED_SAMPLERS[kind].params]


def _make_sampler(kind: int, params):
    """The sampler object of sampler_spec()'s pair."""
    kinds = list(FUSED_SAMPLERS.values())
    if not 0 <= int(kind) < len(kinds) or len(params) != len(kinds[int(kind)].params):
        table = ", ".join(f"{i} = {k.cls.__name__[:-len('Sampler')]} [{', '.join(k.params)}]" for i, k in enumerate(kinds))
        raise RuntimeError(f"mdt::sample_with: sampler_kind {kind} with {len(params)} parameters ({table})")
    k = kinds[int(kind)]
    return k.cls(**dict(zip(k.params, params)))


def _sample(op: str, make_sampler, embedding, init_noise, step_noise, sigmas, handle, pred_dim, sigma_data, embedding_scale,
            clamp, seed, sample0, want_tokens, dynamic_threshold) -> Tuple[Tensor, Tensor]:
    """mdt::sample and mdt::sample_with behind their schemas; ``make_sampler()`` gives the sampler object of the call."""
    dev = _hip(embedding, step_noise)
    eng = _engine_on(handle, dev, op)
    sampler = make_sampler()
    B = embedding.shape[0]
    num_steps = sigmas.numel() - 1
    ns = NoiseSource(seed=int(seed), sample0=int(sample0))
    if init_noise is not None:
        ns.init = init_noise
    if step_noise is not None:
        if step_noise.shape[0] != max(num_steps - 1, 0):
            raise RuntimeError(f"{op}: step_noise holds {step_noise.shape[0]} draws, the loop makes {num_steps - 1}")
        ns.steps = lambda i: step_noise[i]
    tok = torch.zeros(B, eng.c.length, dtype=torch.int32, device=dev) if want_tokens else None
    x = run_sampler(eng, embedding, pred_dim, num_steps, ns, sigmas, sampler, float(sigma_data), float(embedding_scale),
                    bool(clamp), None, None, tok if B else None, float(dynamic_threshold))
    return x, (tok if want_tokens else torch.empty(0, dtype=torch.int32, device=dev))


def _sample_fake(embedding, handle, pred_dim, want_tokens):
    eng = _engine(handle)
    B = embedding.shape[0]
    return (embedding.new_empty(B, pred_dim, eng.c.length, dtype=torch.float32),
            embedding.new_empty((B, eng.c.length) if want_tokens else (0,), dtype=torch.int32))


@custom_op("mdt::sample", mutates_args=())
def sample(embedding: Tensor, init_noise: Optional[Tensor], step_noise: Optional[Tensor], sigmas: Tensor, handle: int,
           pred_dim: int, rho: float, sigma_data: float, embedding_scale: float, clamp: bool, seed: int, sample0: int,
           want_tokens: bool, dynamic_threshold: float = 0.0) -> Tuple[Tensor, Tensor]:
    """The whole ADPM2 loop for an evaluated sigma schedule (num_steps + 1 values).  init_noise (B, C, L) / step_noise
    (num_steps - 1, B, C, L): explicit draws in the reference's call order; each one that is None comes from the counter-based
    generator keyed by (seed, draw index, sample0 + b) instead.  Returns (x (B, C, L), tokens (B, L) int32 or an empty tensor)."""
    return _sample("mdt::sample", lambda: ADPM2Sampler(rho=rho), embedding, init_noise, step_noise, sigmas, handle, pred_dim,
                   sigma_data, embedding_scale, clamp, seed, sample0, want_tokens, dynamic_threshold)


@sample.register_fake
def _(embedding, init_noise, step_noise, sigmas, handle, pred_dim, rho, sigma_data, embedding_scale, clamp, seed, sample0,
      want_tokens, dynamic_threshold=0.0):
    return _sample_fake(embedding, handle, pred_dim, want_tokens)


@custom_op("mdt::sample_with", mutates_args=())
def sample_with(embedding: Tensor, init_noise: Optional[Tensor], step_noise: Optional[Tensor], sigmas: Tensor, handle: int,
                pred_dim: int, sampler_kind: int, sampler_params: Sequence[float], sigma_data: float, embedding_scale: float,
                clamp: bool, seed: int, sample0: int, want_tokens: bool, dynamic_threshold: float = 0.0) -> Tuple[Tensor, Tensor]:
    """mdt::sample with the sampler chosen by the caller: sampler_kind 0 = ADPM2Sampler (sampler_params [rho]), 1 =
    AEulerSampler ([]), 2 = KarrasSampler ([s_tmin, s_tmax, s_churn, s_noise]).  Every other argument and both results as
    mdt::sample; each sampler makes one draw per step, so step_noise has num_steps - 1 draws for all of them."""
    return _sample("mdt::sample_with", lambda: _make_sampler(sampler_kind, list(sampler_params)), embedding, init_noise,
                   step_noise, sigmas, handle, pred_dim, sigma_data, embedding_scale, clamp, seed, sample0, want_tokens,
                   dynamic_threshold)


@sample_with.register_fake
def _(embedding, init_noise, step_noise, sigmas, handle, pred_dim, sampler_kind, sampler_params, sigma_data, embedding_scale,
      clamp, seed, sample0, want_tokens, dynamic_threshold=0.0):
    return _sample_fake(embedding, handle, pred_dim, want_tokens)


@custom_op("mdt::inpaint_tokens", mutates_args=())
def inpaint_tokens(embedding: Tensor, draft: Tensor, keep: Tensor, sigmas: Tensor, handle: int, pred_dim: int,
                   num_resamples: int, rho: float, sigma_data: float, embedding_scale: float, seed: int, sample0: int,
                   dynamic_threshold: float = 0.0) -> Tuple[Tensor, Tensor]:
    """The whole ADPM2 inpainting loop (ADPM2Sampler.inpaint, diffusion.py:526-549) for an evaluated sigma schedule (num_steps + 1
    values) on a draft given as token ids: draft (B, L) integer ids in [0, pred_dim) standing for their +-1 one-hot, keep (B, L)
    bool, True = keep the position.  Every draw comes from the counter-based generator keyed by (seed, draw index, sample0 + b).
    Returns (x (B, pred_dim, L) fp32, tokens (B, L) int32: argmax over channels, the draft id at a kept position)."""
    dev = _hip(embedding, draft, keep)
    eng = _engine_on(handle, dev, "mdt::inpaint_tokens")
    B = embedding.shape[0]
    if draft.is_floating_point() or keep.dtype != torch.bool or tuple(draft.shape) != (B, eng.c.length) or keep.shape != draft.shape:
        raise RuntimeError(f"mdt::inpaint_tokens: draft must be integer ids and keep bool, both ({B}, {eng.c.length}); got "
                           f"{draft.dtype} {tuple(draft.shape)} and {keep.dtype} {tuple(keep.shape)}")
    tok = torch.zeros(B, eng.c.length, dtype=torch.int32, device=dev)
    if B == 0:
        return torch.empty(0, pred_dim, eng.c.length, device=dev), tok
    x = run_adpm2_inpaint(eng, embedding, None, None, sigmas.numel() - 1, int(num_resamples), None, int(seed), sigmas,
                          ADPM2Sampler(rho=rho), float(sigma_data), float(embedding_scale), int(sample0), float(dynamic_threshold),
                          draft=draft, keep=keep, pred_dim=int(pred_dim), tokens=tok)
    return x, tok


@inpaint_tokens.register_fake
def _(embedding, draft, keep, sigmas, handle, pred_dim, num_resamples, rho, sigma_data, embedding_scale, seed, sample0,
      dynamic_threshold=0.0):
    B, L = draft.shape
    return embedding.new_empty(B, pred_dim, L, dtype=torch.float32), draft.new_empty((B, L), dtype=torch.int32)


@custom_op("mdt::refine_tokens", mutates_args=())
def refine_tokens(embedding: Tensor, draft: Tensor, start: Tensor, init_noise: Optional[Tensor], sigmas: Tensor, handle: int,
                  pred_dim: int, sampler_kind: int, sampler_params: Sequence[float], sigma_data: float, embedding_scale: float,
                  seed: int, sample0: int, dynamic_threshold: float = 0.0) -> Tuple[Tensor, Tensor]:
    """The whole refine loop (diffusion.run_refine) for an evaluated sigma schedule (num_steps + 1 values) on a draft given as
    token ids: draft (B, L) integer ids in [0, pred_dim) standing for their +-1 one-hot, start (B,) int32 in [0, num_steps - 2]:
    row b is ``one_hot(draft[b]) + sigmas[start[b]] * draw0[b]`` followed by steps start[b] .. num_steps - 2 of the sampler
    (sampler_kind / sampler_params as mdt::sample_with).  init_noise (B, pred_dim, L): the entry noise, or None; it and every step
    draw otherwise come from the counter-based generator keyed by (seed, draw index, sample0 + b), draw 0 = the entry, draw i + 1 =
    step i.  Returns (x (B, pred_dim, L) fp32, tokens (B, L) int32: argmax over channels)."""
    dev = _hip(embedding, draft, start, init_noise)
    eng = _engine_on(handle, dev, "mdt::refine_tokens")
    B, L = embedding.shape[0], eng.c.length
    if draft.is_floating_point() or tuple(draft.shape) != (B, L) or start.dtype != torch.int32 or tuple(start.shape) != (B,):
        raise RuntimeError(f"mdt::refine_tokens: draft must be integer ids ({B}, {L}) and start int32 ({B},); got {draft.dtype} "
                           f"{tuple(draft.shape)} and {start.dtype} {tuple(start.shape)}")
    if init_noise is not None and tuple(init_noise.shape) != (B, pred_dim, L):
        raise RuntimeError(f"mdt::refine_tokens: init_noise is {tuple(init_noise.shape)}, not ({B}, {pred_dim}, {L})")
    tok = torch.zeros(B, L, dtype=torch.int32, device=dev)
    if B == 0:
        return torch.empty(0, pred_dim, L, device=dev), tok
    ns = NoiseSource(seed=int(seed), sample0=int(sample0))
    if init_noise is not None:
        ns.init = init_noise
    try:
        x = run_refine(eng, embedding, int(pred_dim), sigmas.numel() - 1, ns, sigmas, _make_sampler(sampler_kind, list(sampler_params)),
                       float(sigma_data), start.cpu(), draft=draft, embedding_scale=float(embedding_scale), tokens=tok,
                       dynamic_threshold=float(dynamic_threshold))
    except ValueError as e:                      # (the ops' convention: every failure is a RuntimeError)
        raise RuntimeError(f"mdt::refine_tokens: {e}") from None
    return x, tok


@refine_tokens.register_fake
def _(embedding, draft, start, init_noise, sigmas, handle, pred_dim, sampler_kind, sampler_params, sigma_data, embedding_scale,
      seed, sample0, dynamic_threshold=0.0):
    B, L = draft.shape
    return embedding.new_empty(B, pred_dim, L, dtype=torch.float32), draft.new_empty((B, L), dtype=torch.int32)


@custom_op("mdt::refine_keep_tokens", mutates_args=())
def refine_keep_tokens(embedding: Tensor, draft: Tensor, start: Tensor, keep: Tensor, init_noise: Optional[Tensor], sigmas: Tensor,
                       handle: int, pred_dim: int, sampler_kind: int, sampler_params: Sequence[float], sigma_data: float,
                       embedding_scale: float, seed: int, sample0: int, dynamic_threshold: float = 0.0) -> Tuple[Tensor, Tensor]:
    """mdt::refine_tokens around a kept scaffold (diffusion.run_refine with ``keep``): keep (B, L) bool, True = the position is
    re-noised from the draft in front of every step and is the draft in the result.  The source draw of step i is draw
    num_steps + i of the generator; the other arguments and draws as mdt::refine_tokens.  Returns (x (B, pred_dim, L) fp32 with
    the one-hot of the draft at the kept positions, tokens (B, L) int32: the draft id at a kept position, else the argmax)."""
    dev = _hip(embedding, draft, start, keep, init_noise)
    eng = _engine_on(handle, dev, "mdt::refine_keep_tokens")
    B, L = embedding.shape[0], eng.c.length
    if draft.is_floating_point() or tuple(draft.shape) != (B, L) or start.dtype != torch.int32 or tuple(start.shape) != (B,):
        raise RuntimeError(f"mdt::refine_keep_tokens: draft must be integer ids ({B}, {L}) and start int32 ({B},); got {draft.dtype} "
                           f"{tuple(draft.shape)} and {start.dtype} {tuple(start.shape)}")
    if keep.dtype != torch.bool or tuple(keep.shape) != (B, L):
        raise RuntimeError(f"mdt::refine_keep_tokens: keep must be bool ({B}, {L}); got {keep.dtype} {tuple(keep.shape)}")
    if init_noise is not None and tuple(init_noise.shape) != (B, pred_dim, L):
        raise RuntimeError(f"mdt::refine_keep_tokens: init_noise is {tuple(init_noise.shape)}, not ({B}, {pred_dim}, {L})")
    tok = torch.zeros(B, L, dtype=torch.int32, device=dev)
    if B == 0:
        return torch.empty(0, pred_dim, L, device=dev), tok
    ns = NoiseSource(seed=int(seed), sample0=int(sample0))
    if init_noise is not None:
        ns.init = init_noise
    try:
        x = run_refine(eng, embedding, int(pred_dim), sigmas.numel() - 1, ns, sigmas, _make_sampler(sampler_kind, list(sampler_params)),
                       float(sigma_data), start.cpu(), draft=draft, embedding_scale=float(embedding_scale), tokens=tok,
                       dynamic_threshold=float(dynamic_threshold), keep=keep, keep_per_token=True)
    except ValueError as e:                      # (the ops' convention: every failure is a RuntimeError)
        raise RuntimeError(f"mdt::refine_keep_tokens: {e}") from None
    return x, tok


@refine_keep_tokens.register_fake
def _(embedding, draft, start, keep, init_noise, sigmas, handle, pred_dim, sampler_kind, sampler_params, sigma_data, embedding_scale,
      seed, sample0, dynamic_threshold=0.0):
    B, L = draft.shape
    return embedding.new_empty(B, pred_dim, L, dtype=torch.float32), draft.new_empty((B, L), dtype=torch.int32)


@custom_op("mdt::all_gather_samples", mutates_args=())
def all_gather_samples(local: Tensor, total: int) -> Tensor:
    """(b_r, ...) per rank -> (total, ...) on every rank over the default process group (RCCL on HIP tensors)."""
    from .distributed import all_gather_samples as gather
    return gather(local, int(total), force_collective=True)


@all_gather_samples.register_fake
def _(local, total):
    return local.new_empty((total,) + tuple(local.shape[1:]))
