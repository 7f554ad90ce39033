"""k-diffusion runtime of the sampling path: Karras schedule, the ADPM2 / AEuler / Karras samplers, KDiffusion_mod
preconditioning, kept behind the reference's class seams (diffusion.py:324-342, :399-549, :554-625,
:706-814) while the per-step arithmetic runs in the fused HIP kernels of libmdt_hip.so.

Host side = scalar bookkeeping only.  All per-step scalars are computed up front in exactly the mixed
precision the reference uses (0-dim fp32 tensors, Python doubles through math.sqrt), which
removes the >= 4 device->host synchronisations per step of the reference loop.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Callable, List, NamedTuple, Optional, Union

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import runtime as rt

Tensor = torch.Tensor


# ----------------------------------------------------------------------------------------------
# distributions / schedules / samplers (constructor-compatible with the reference classes)
# ----------------------------------------------------------------------------------------------
class LogNormalDistribution:
    """diffusion.py:29-38 (training-time sigma sampling; not used by sample())."""

    def __init__(self, mean: float, std: float):
        self.mean, self.std = mean, std

    def __call__(self, num_samples: int, device=torch.device("cpu")) -> Tensor:
        return (self.mean + self.std * torch.randn((num_samples,), device=device)).exp()


class KarrasSchedule(nn.Module):
    """diffusion.py:324-342.  Evaluated on the host (CPU fp32), as the reference's CPU path does."""

    def __init__(self, sigma_min: float, sigma_max: float, rho: float = 7.0):
        super().__init__()
        self.sigma_min, self.sigma_max, self.rho = sigma_min, sigma_max, rho

    def forward(self, num_steps: int, device=None) -> Tensor:
        rho_inv = 1.0 / self.rho
        steps = torch.arange(num_steps, dtype=torch.float32)
        sigmas = (self.sigma_max ** rho_inv
                  + (steps / (num_steps - 1)) * (self.sigma_min ** rho_inv - self.sigma_max ** rho_inv)) ** self.rho
        return F.pad(sigmas, pad=(0, 1), value=0.0)


class _KAlias:
    """Stands for the reference's diffusion classes in Sampler.diffusion_types (only their alias is consulted,
    diffusion.py:571-575)."""

    def __init__(self, alias: str):
        self.alias = alias


class Sampler(nn.Module):
    """diffusion.py:347-366."""

    diffusion_types: list = []

    def forward(self, noise: Tensor, fn: Callable, sigmas: Tensor, num_steps: int) -> Tensor:
        raise NotImplementedError()

    def inpaint(self, source: Tensor, mask: Tensor, fn: Callable, sigmas: Tensor, num_steps: int,
                num_resamples: int) -> Tensor:
        raise NotImplementedError("Inpainting not available with current sampler")


def _step_inputs(name: str, x: Tensor, sigma, sigma_next):
    """What every per-step path starts from: the two sigmas as 0-dim fp32 CPU tensors (the reference indexes a CPU schedule)
    and the state as a contiguous fp32 HIP tensor."""
    if x.device.type != "cuda":
        raise RuntimeError(f"{name}.step runs on an AMD GPU through libmdt_hip.so (no CPU fallback)")
    sigma = torch.as_tensor(sigma, dtype=torch.float32).cpu().reshape(())
    sigma_next = torch.as_tensor(sigma_next, dtype=torch.float32).cpu().reshape(())
    return x.detach().float().contiguous(), sigma, sigma_next


def _step_draw(x: Tensor, noise: Optional[Tensor]) -> Tensor:
    """The torch.randn_like(x) draw of a step (diffusion.py:514), or the caller's tensor in its place."""
    return (torch.randn_like(x) if noise is None else noise.to(device=x.device, dtype=torch.float32)).contiguous()


class _LoopSampler(Sampler):
    """forward() of the three samplers built here.  With the denoiser of a QMDiffusion* model (BoundDenoise.fused) the whole
    loop runs on the fused path (run_sampler); with any other ``fn``, or in a subclass that overrides step() (it is honoured),
    forward() calls step() once per timestep as the reference does."""

    diffusion_types = [_KAlias("k"), _KAlias("vk")]

    def _fused(self, fn: Callable):
        return getattr(fn, "fused", None) if fused_sampler_kind(self) else None

    def _step_args(self, sigmas: Tensor, num_steps: int):
        """(the sigmas step() is given, i -> the keyword arguments of step i beyond the two sigmas)."""
        return sigmas, lambda i: {}

    def forward(self, noise, fn: Callable, sigmas: Tensor, num_steps: int) -> Tensor:
        """diffusion.py:437-453, :476-483, :517-524.  ``noise`` is the initial draw (B, C, L) or, on the fused path, a
        NoiseSource."""
        fused = self._fused(fn)
        if fused is not None:
            return fused.sample(noise, self, sigmas, num_steps)
        if isinstance(noise, NoiseSource):
            raise TypeError("a NoiseSource drives the fused path only; pass the initial noise tensor with a custom fn")
        x = float(sigmas[0]) * noise
        sigmas, extra = self._step_args(sigmas, num_steps)
        for i in range(num_steps - 1):
            x = self.step(x, fn=fn, sigma=sigmas[i], sigma_next=sigmas[i + 1], **extra(i))
        return x


class ADPM2Sampler(_LoopSampler):
    """diffusion.py:486-549: second-order ancestral DPM-2 sampler.

    ``fn(x, sigma=...)`` is any denoiser on HIP tensors.  When it is the denoiser of a QMDiffusion* model (the closure
    DiffusionSampler / DiffusionInpainter build), forward()/inpaint() run the whole loop on the fused path (run_sampler /
    run_adpm2_inpaint: per-step scalars precomputed on the host, preconditioning + update fused, the U-Net as a replayed HIP
    graph); with any other ``fn`` every step is two calls of ``fn`` and two mdt_adpm2_euler launches (the reference's
    arithmetic, fp32, no contraction), drawing the step noise with torch.randn_like on the device exactly as
    diffusion.py:514 does."""

    def __init__(self, rho: float = 1.0):
        super().__init__()
        self.rho = rho

    def get_sigmas(self, sigma, sigma_next):
        r = self.rho
        sigma_up = math.sqrt(sigma_next ** 2 * (sigma ** 2 - sigma_next ** 2) / sigma ** 2)
        sigma_down = math.sqrt(sigma_next ** 2 - sigma_up ** 2)
        sigma_mid = ((sigma ** (1 / r) + sigma_down ** (1 / r)) / 2) ** r
        return sigma_up, sigma_down, sigma_mid

    def step(self, x: Tensor, fn: Callable, sigma, sigma_next, *, noise: Optional[Tensor] = None) -> Tensor:
        """diffusion.py:502-515 for one step; ``noise`` replaces the torch.randn_like(x) draw (parity tests)."""
        lib = rt.load_library()
        x, sigma, sigma_next = _step_inputs("ADPM2Sampler", x, sigma, sigma_next)
        sigma_up, sigma_down, sigma_mid = self.get_sigmas(sigma, sigma_next)
        dt_mid, dt_down = float(sigma_mid - sigma), float(sigma_down - sigma)     # fp32 tensor arithmetic, as the reference
        up32 = float(torch.tensor(sigma_up, dtype=torch.float32))
        B, C, L = x.shape
        with torch.no_grad(), torch.cuda.device(x.device):
            st = rt.current_stream()
            den = fn(x, sigma=sigma).float().contiguous()
            x_mid = torch.empty_like(x)
            rt.check(lib.mdt_adpm2_euler(rt.ptr(x), rt.ptr(x), rt.ptr(den), 0, rt.ptr(x_mid), float(sigma), dt_mid, 0.0, 0,
                                         0, 0, 0, B, C, L, st))
            den_mid = fn(x_mid, sigma=torch.as_tensor(sigma_mid, dtype=torch.float32)).float().contiguous()
            nz = _step_draw(x, noise)
            out = torch.empty_like(x)
            rt.check(lib.mdt_adpm2_euler(rt.ptr(x), rt.ptr(x_mid), rt.ptr(den_mid), rt.ptr(nz), rt.ptr(out),
                                         float(sigma_mid), dt_down, up32, 1, 0, 0, 0, B, C, L, st))
        return out

    def inpaint(self, source: Tensor, mask: Tensor, fn: Callable, sigmas: Tensor, num_steps: int,
                num_resamples: int) -> Tensor:
        """diffusion.py:526-549."""
        fused = self._fused(fn)
        if fused is not None:
            return fused.inpaint(source, mask, self, sigmas, num_steps, num_resamples)
        if not source.is_floating_point():
            raise TypeError("draft token ids drive the fused path only; pass the one-hot draft (one_hot_draft) with a custom fn")
        x = float(sigmas[0]) * torch.randn_like(source)
        for i in range(num_steps - 1):
            source_noisy = source + float(sigmas[i]) * torch.randn_like(source)
            for r in range(num_resamples):
                x = source_noisy * mask + x * ~mask
                x = self.step(x, fn=fn, sigma=sigmas[i], sigma_next=sigmas[i + 1])
                if r < num_resamples - 1:
                    sigma = math.sqrt(sigmas[i] ** 2 - sigmas[i + 1] ** 2)
                    x = x + sigma * torch.randn_like(x)
        return source * mask + x * ~mask


class AEulerSampler(_LoopSampler):
    """diffusion.py:456-483: ancestral Euler sampler, ONE evaluation per step (ADPM2 and Karras take two).

    Same seams as ADPM2Sampler: with the denoiser of a QMDiffusion* model forward() runs the whole loop on the fused path
    (_aeuler_steps: one mdt_aeuler_next launch per step around the replayed U-Net graph); with any other ``fn`` every step is
    one call of ``fn`` and one mdt_adpm2_euler launch.  inpaint() is the base class's NotImplementedError, as in the
    reference."""

    def get_sigmas(self, sigma, sigma_next):
        sigma_up = math.sqrt(sigma_next ** 2 * (sigma ** 2 - sigma_next ** 2) / sigma ** 2)
        sigma_down = math.sqrt(sigma_next ** 2 - sigma_up ** 2)
        return sigma_up, sigma_down

    def step(self, x: Tensor, fn: Callable, sigma, sigma_next, *, noise: Optional[Tensor] = None) -> Tensor:
        """diffusion.py:465-474 for one step; ``noise`` replaces the torch.randn_like(x) draw (parity tests)."""
        lib = rt.load_library()
        x, sigma, sigma_next = _step_inputs("AEulerSampler", x, sigma, sigma_next)
        sigma_up, sigma_down = self.get_sigmas(sigma, sigma_next)
        dt = float(sigma_down - sigma)                                             # fp32 tensor arithmetic, as the reference
        up32 = float(torch.tensor(sigma_up, dtype=torch.float32))
        B, C, L = x.shape
        with torch.no_grad(), torch.cuda.device(x.device):
            den = fn(x, sigma=sigma).float().contiguous()
            nz = _step_draw(x, noise)
            out = torch.empty_like(x)
            rt.check(lib.mdt_adpm2_euler(rt.ptr(x), rt.ptr(x), rt.ptr(den), rt.ptr(nz), rt.ptr(out), float(sigma), dt, up32, 1,
                                         0, 0, 0, B, C, L, rt.current_stream()))
        return out


class KarrasSampler(_LoopSampler):
    """diffusion.py:399-453: the stochastic second-order sampler of Karras et al. (arXiv:2206.00364, algorithm 2) AS THE
    REFERENCE WRITES IT.  Its correction line is ``x_next = x_hat + 0.5 * (sigma - sigma_hat) * (d + d_prime)`` (:434), not
    the paper's ``x_hat + 0.5 * (sigma_next - sigma_hat) * (d + d_prime)``: without churn (gamma = 0, the constructor's
    default) sigma_hat == sigma and every step returns x_hat = x, so ``KarrasSampler()`` returns ``sigmas[0] * noise`` bit
    for bit; with churn a step moves x by ``-0.5 gamma sigma (d + d')`` only.  This package reproduces the reference's
    arithmetic, so it does the same (pinned by tests/golden/tiny_b3_t8_karras0_sample.npz); it is not "fixed" here.

    With the denoiser of a QMDiffusion* model forward() runs the fused loop (_karras_steps: mdt_karras_hat / _mid / _next
    around the two evaluations of a step); with any other ``fn`` a step is two calls of ``fn`` plus elementwise launches."""

    def __init__(self, s_tmin: float = 0, s_tmax: float = float("inf"), s_churn: float = 0.0, s_noise: float = 1.0):
        super().__init__()
        self.s_tmin = s_tmin
        self.s_tmax = s_tmax
        self.s_noise = s_noise
        self.s_churn = s_churn

    def get_gammas(self, sigmas: Tensor, num_steps: int) -> Tensor:
        """The gammas of forward() (diffusion.py:442-446), one per entry of ``sigmas``."""
        return torch.where((sigmas >= self.s_tmin) & (sigmas <= self.s_tmax),
                           min(self.s_churn / num_steps, math.sqrt(2) - 1), 0.0)

    def step(self, x: Tensor, fn: Callable, sigma, sigma_next, gamma, *, noise: Optional[Tensor] = None) -> Tensor:
        """diffusion.py:417-435 for one step; ``noise`` replaces the torch.randn_like(x) draw (parity tests)."""
        lib = rt.load_library()
        x, sigma, sigma_next = _step_inputs("KarrasSampler", x, sigma, sigma_next)
        gamma = torch.as_tensor(gamma, dtype=torch.float32).cpu().reshape(())
        sigma_hat = sigma + gamma * sigma
        ns32 = float(torch.tensor(math.sqrt(sigma_hat ** 2 - sigma ** 2), dtype=torch.float32))
        s_noise32 = float(torch.tensor(self.s_noise, dtype=torch.float32))
        dt, half = float(sigma_next - sigma_hat), float(0.5 * (sigma - sigma_hat))    # fp32 tensor arithmetic, as the reference
        B, C, L = x.shape
        with torch.no_grad(), torch.cuda.device(x.device):
            st = rt.current_stream()
            nz = _step_draw(x, noise)
            eps = (s_noise32 * nz).contiguous()
            x_hat = x.clone()
            rt.check(lib.mdt_add_noise(rt.ptr(x_hat), rt.ptr(eps), ns32, 0, 0, 0, B, C, L, st))
            den = fn(x_hat, sigma=sigma_hat).float().contiguous()
            x_next = torch.empty_like(x)
            rt.check(lib.mdt_adpm2_euler(rt.ptr(x_hat), rt.ptr(x_hat), rt.ptr(den), 0, rt.ptr(x_next), float(sigma_hat), dt, 0.0,
                                         0, 0, 0, 0, B, C, L, st))
            if sigma_next != 0:
                den_next = fn(x_next, sigma=sigma_next).float()
                # (0-dim DEVICE divisors: a host scalar would turn the division into a multiplication by its reciprocal)
                d = (x_hat - den) / sigma_hat.to(x.device)
                d_prime = (x_next - den_next) / sigma_next.to(x.device)
                x_next = x_hat + half * (d + d_prime)
        return x_next

    def _step_args(self, sigmas: Tensor, num_steps: int):
        sigmas = torch.as_tensor(sigmas, dtype=torch.float32).cpu()
        gammas = self.get_gammas(sigmas, num_steps)
        return sigmas, lambda i: dict(gamma=gammas[i])


def fused_sampler_kind(sampler) -> Optional[str]:
    """'adpm2' | 'aeuler' | 'karras' when ``sampler`` may take the fused loop of a QMDiffusion* model -- one of the three
    sampler classes with its own step() (a subclass that overrides step() is honoured: it gets the per-step path) -- else None."""
    for kind, k in FUSED_SAMPLERS.items():
        if isinstance(sampler, k.cls):
            return kind if type(sampler).step is k.cls.step else None
    return None


@dataclass
class ScaleWeights:
    c_skip: float
    c_out: float
    c_in: float
    c_noise: float


def scale_weights(sigma: Tensor, sigma_data: float) -> ScaleWeights:
    """KDiffusion_mod.get_scale_weights (diffusion.py:789-796) for one sigma (0-dim fp32 tensor),
    evaluated as the reference does on a to_batch()-ed fp32 vector (diffusion.py:91-102)."""
    sigmas = torch.as_tensor(sigma, dtype=torch.float32).reshape(1).expand(16).clone()
    c_noise = torch.log(sigmas) * 0.25
    s = sigmas.view(-1, 1, 1)
    c_skip = (sigma_data ** 2) / (s ** 2 + sigma_data ** 2)
    c_out = s * sigma_data * (sigma_data ** 2 + s ** 2) ** -0.5
    c_in = (s ** 2 + sigma_data ** 2) ** -0.5
    return ScaleWeights(float(c_skip.flatten()[0]), float(c_out.flatten()[0]), float(c_in.flatten()[0]),
                        float(c_noise[0]))


@dataclass(frozen=True)
class RowWeights:
    """get_scale_weights + loss_weight (diffusion.py:789-796, :816-818) for one sigma PER SAMPLE: fp32 CPU vectors of B entries."""
    sigmas: Tensor
    c_skip: Tensor
    c_out: Tensor
    c_in: Tensor
    c_noise: Tensor
    loss_weight: Tensor

    def packed(self) -> Tensor:
        """(6, B): sigma | c_in | c_skip | c_out | c_noise | loss_weight -- one upload per call."""
        return torch.stack((self.sigmas, self.c_in, self.c_skip, self.c_out, self.c_noise, self.loss_weight))


def scale_weights_rows(sigmas: Tensor, sigma_data: float) -> RowWeights:
    """The per-sample form of scale_weights: the reference's fp32 tensor expressions on the whole sigma vector
    (KDiffusion_mod.forward, diffusion.py:820-844).  Element i equals scale_weights(sigmas[i]) bit for bit: the vector is padded to
    a multiple of 16 entries, so every element takes the vectorised path that scale_weights' 16-entry vector takes."""
    sig = torch.as_tensor(sigmas, dtype=torch.float32).flatten().cpu()
    n = sig.numel()
    pad = torch.ones((n + 15) // 16 * 16, dtype=torch.float32)
    pad[:n] = sig
    c_noise = torch.log(pad) * 0.25
    s = pad.view(-1, 1, 1)
    c_skip = (sigma_data ** 2) / (s ** 2 + sigma_data ** 2)
    c_out = s * sigma_data * (sigma_data ** 2 + s ** 2) ** -0.5
    c_in = (s ** 2 + sigma_data ** 2) ** -0.5
    weight = (pad ** 2 + sigma_data ** 2) * (pad * sigma_data) ** -2
    return RowWeights(sig, c_skip.flatten()[:n].clone(), c_out.flatten()[:n].clone(), c_in.flatten()[:n].clone(),
                      c_noise[:n].clone(), weight[:n].clone())


@dataclass(frozen=True)
class StepScalars:
    """Everything one ADPM2 step needs, as fp32-exact Python floats."""
    sigma: float
    sigma_mid: float
    sigma_up: float          # fp32(sigma_up): `randn * sigma_up` multiplies by the double cast to fp32
    dt_mid: float            # fp32(sigma_mid - sigma)
    dt_down: float           # fp32(sigma_down - sigma)
    w: ScaleWeights          # at sigma
    w_mid: ScaleWeights      # at sigma_mid
    renoise: float           # sqrt(sigma^2 - sigma_next^2) for inpaint resampling (diffusion.py:546)


_PLAN_CACHE: dict = {}


def _cached_plan(num_steps: int, schedule, sampler, params: tuple, sigma_data: float, make_steps: Callable):
    """(sigmas, steps) of a plan function: ``make_steps(sigmas)`` yields the per-step scalars when the cache has none.
    A plan is a pure function of (sigmas, sampler class and ``params``, sigma_data) and costs ~10 ms of 0-dim tensor arithmetic
    for 64 timesteps (it has to: the reference's mixed double / fp32 rounding is reproduced op by op).  Hidden while the GPU
    queue is full, but a call that waits for its hand-off status (engine.note_handoff) exposes the NEXT call's host prologue:
    keep the last plans."""
    sigmas = schedule.detach().float().cpu() if isinstance(schedule, torch.Tensor) else schedule(num_steps)
    key = (num_steps, sigmas.numpy().tobytes(), type(sampler), params, float(sigma_data))
    steps = _PLAN_CACHE.get(key)
    if steps is None:
        steps = tuple(make_steps(sigmas))                # (a tuple: every caller shares it)
        if len(_PLAN_CACHE) >= 16:
            _PLAN_CACHE.pop(next(iter(_PLAN_CACHE)))
        _PLAN_CACHE[key] = steps
    return sigmas, steps


def adpm2_plan(num_steps: int, schedule, sampler: ADPM2Sampler, sigma_data: float):
    """Per-step scalars of ADPM2Sampler.forward/step (diffusion.py:502-524), bit-for-bit as the reference
    computes them on CPU.  ``schedule`` is a KarrasSchedule or an already evaluated (num_steps + 1,) sigma tensor."""
    def make_steps(sigmas):
        for i in range(num_steps - 1):
            sigma, sigma_next = sigmas[i], sigmas[i + 1]
            sigma_up, sigma_down, sigma_mid = sampler.get_sigmas(sigma, sigma_next)
            dt_mid = sigma_mid - sigma                       # 0-dim fp32
            dt_down = sigma_down - sigma                     # python double - fp32 tensor -> fp32 tensor
            up32 = torch.tensor(sigma_up, dtype=torch.float32)
            renoise = math.sqrt(sigmas[i] ** 2 - sigmas[i + 1] ** 2)
            yield StepScalars(float(sigma), float(sigma_mid), float(up32), float(dt_mid), float(dt_down),
                              scale_weights(sigma, sigma_data), scale_weights(sigma_mid, sigma_data),
                              float(torch.tensor(renoise, dtype=torch.float32)))
    return _cached_plan(num_steps, schedule, sampler, (float(getattr(sampler, "rho", 0.0)),), sigma_data, make_steps)


@dataclass(frozen=True)
class AEulerStep:
    """Everything one AEulerSampler step needs, as fp32-exact Python floats."""
    sigma: float
    sigma_up: float          # fp32(sigma_up)
    dt: float                # fp32(sigma_down - sigma)
    w: ScaleWeights          # at sigma


@dataclass(frozen=True)
class KarrasStep:
    """Everything one KarrasSampler step needs, as fp32-exact Python floats."""
    sigma: float
    sigma_next: float
    gamma: float
    sigma_hat: float         # sigma + gamma * sigma
    noise_scale: float       # fp32(sqrt(sigma_hat^2 - sigma^2))
    s_noise: float           # fp32(s_noise)
    dt: float                # sigma_next - sigma_hat
    half: float              # 0.5 * (sigma - sigma_hat): the factor of the reference's correction line (diffusion.py:434)
    w_hat: ScaleWeights      # at sigma_hat
    w_next: Optional[ScaleWeights]   # at sigma_next; None when euler_only
    euler_only: bool         # sigma_next == 0: no second evaluation, no correction (diffusion.py:431)
    row_hat: int             # rows of the call's time table (c_noise of every evaluation, in order)
    row_next: int            # -1 when euler_only


def aeuler_plan(num_steps: int, schedule, sampler: AEulerSampler, sigma_data: float):
    """Per-step scalars of AEulerSampler.forward/step (diffusion.py:465-483), bit for bit as the reference computes them on
    CPU; ``schedule`` and the cache as adpm2_plan.  One time row per step."""
    def make_steps(sigmas):
        for i in range(num_steps - 1):
            sigma, sigma_next = sigmas[i], sigmas[i + 1]
            sigma_up, sigma_down = sampler.get_sigmas(sigma, sigma_next)
            dt = sigma_down - sigma                          # python double - fp32 tensor -> fp32 tensor
            up32 = torch.tensor(sigma_up, dtype=torch.float32)
            yield AEulerStep(float(sigma), float(up32), float(dt), scale_weights(sigma, sigma_data))
    return _cached_plan(num_steps, schedule, sampler, (), sigma_data, make_steps)


def karras_plan(num_steps: int, schedule, sampler: KarrasSampler, sigma_data: float):
    """Per-step scalars of KarrasSampler.forward/step (diffusion.py:417-453), bit for bit as the reference computes them on
    CPU; ``schedule`` and the cache as adpm2_plan.  Two time rows per step, one when sigma_next == 0 (reachable with an
    evaluated sigma tensor that ends in 0; a KarrasSchedule's padded 0 is never reached)."""
    def make_steps(sigmas):
        gammas = sampler.get_gammas(sigmas, num_steps)
        s_noise32 = float(torch.tensor(sampler.s_noise, dtype=torch.float32))     # python double * fp32 tensor: rounded first
        rows = 0
        for i in range(num_steps - 1):
            sigma, sigma_next, gamma = sigmas[i], sigmas[i + 1], gammas[i]
            sigma_hat = sigma + gamma * sigma                                     # 0-dim fp32
            ns32 = torch.tensor(math.sqrt(sigma_hat ** 2 - sigma ** 2), dtype=torch.float32)
            dt = sigma_next - sigma_hat
            half = 0.5 * (sigma - sigma_hat)
            euler_only = not bool(sigma_next != 0)
            yield KarrasStep(float(sigma), float(sigma_next), float(gamma), float(sigma_hat), float(ns32), s_noise32,
                             float(dt), float(half), scale_weights(sigma_hat, sigma_data),
                             None if euler_only else scale_weights(sigma_next, sigma_data), euler_only,
                             rows, -1 if euler_only else rows + 1)
            rows += 1 if euler_only else 2
    params = (float(sampler.s_tmin), float(sampler.s_tmax), float(sampler.s_churn), float(sampler.s_noise))
    return _cached_plan(num_steps, schedule, sampler, params, sigma_data, make_steps)


def plan_time_rows(steps) -> List[float]:
    """c_noise of every U-Net evaluation of a planned call, in evaluation order (the rows engine.prepare_times fills)."""
    rows: List[float] = []
    for s in steps:
        if isinstance(s, StepScalars):
            rows += [s.w.c_noise, s.w_mid.c_noise]
        elif isinstance(s, AEulerStep):
            rows.append(s.w.c_noise)
        else:
            rows.append(s.w_hat.c_noise)
            if not s.euler_only:
                rows.append(s.w_next.c_noise)
    return rows


class NoiseSource:
    """Where torch.randn / torch.randn_like of the reference come from.

    * explicit tensors (parity mode): ``init`` is the (B, C, L) draw of generative.py:853, ``steps(i)``
      returns the torch.randn_like draw of step i (diffusion.py:514) already on the device;
    * ``seed`` (throughput mode): on-device Philox4x32-10 keyed by (seed, draw index) with the counter
      taken from the GLOBAL sample index ``sample0 + b`` so results do not depend on the sharding.

    ``sources(i)`` (explicit mode, a refine call with a keep mask only): the torch.randn_like draw that noises the kept source in
    front of step i (diffusion.py:539), already on the device.
    """

    def __init__(self, init: Optional[Tensor] = None, steps: Optional[Callable[[int], Tensor]] = None,
                 seed: Optional[int] = None, sample0: int = 0, sources: Optional[Callable[[int], Tensor]] = None):
        if (init is None) != (steps is None) or (init is None) == (seed is None):
            raise ValueError("give either (init, steps) tensors or a seed")
        self.init, self.steps, self.seed, self.sample0, self.sources = init, steps, seed, sample0, sources


class BoundDenoise:
    """The closure ``fn = lambda *a, **ka: denoise_fn(*a, **{**ka, **kwargs})`` of DiffusionSampler.forward /
    DiffusionInpainter.forward (diffusion.py:587, :614) as an object: calling it evaluates the denoiser; ``fused`` is the
    owning model's fused-loop adapter when the denoiser is a QMDiffusion* model's (else None), which lets
    ADPM2Sampler.forward / inpaint take the whole loop instead of calling back per step."""

    def __init__(self, denoise_fn: Callable, kwargs: dict, extra: Optional[dict] = None):
        self.denoise_fn, self.kwargs, self._extra = denoise_fn, dict(kwargs), dict(extra or {})
        self._owner = getattr(getattr(denoise_fn, "__self__", None), "_owner", None)
        self._fused = False            # not built yet

    @property
    def fused(self):
        """Built on first use (a custom Sampler that only calls back per step never needs it); None when the denoiser is
        not a QMDiffusion* model's, or when the call carries kwargs the fused loop does not take (they then reach
        denoise_fn through the per-step path, which raises or accepts them exactly as the callable does)."""
        if self._fused is False:
            self._fused = None
            if self._owner is not None:
                try:
                    self._fused = self._owner._fused_adapter(self.kwargs, self._extra)
                except TypeError:
                    self._fused = None
        return self._fused

    def __call__(self, *a, **ka):
        return self.denoise_fn(*a, **{**ka, **self.kwargs})


class DiffusionSampler(nn.Module):
    """diffusion.py:554-591."""

    def __init__(self, diffusion, *, sampler: Sampler, sigma_schedule, num_steps: Optional[int] = None, clamp: bool = True):
        super().__init__()
        self.denoise_fn = diffusion.denoise_fn
        self.sampler = sampler
        self.sigma_schedule = sigma_schedule
        self.num_steps = num_steps
        self.clamp = clamp
        message = f"{sampler.__class__.__name__} incompatible with {diffusion.__class__.__name__}"
        assert diffusion.alias in [t.alias for t in sampler.diffusion_types], message

    @torch.no_grad()
    def forward(self, noise, num_steps: Optional[int] = None, *, trace=None, timer=None, tokens=None, **kwargs) -> Tensor:
        num_steps = self.num_steps if num_steps is None else num_steps
        assert num_steps is not None, "Parameter `num_steps` must be provided"
        device = kwargs["embedding"].device if isinstance(kwargs.get("embedding"), torch.Tensor) else None
        sigmas = self.sigma_schedule(num_steps, device)             # diffusion.py:585: (num_steps, device)
        fn = BoundDenoise(self.denoise_fn, kwargs, dict(trace=trace, timer=timer, tokens=tokens, clamp=self.clamp))
        x = self.sampler(noise, fn=fn, sigmas=sigmas, num_steps=num_steps)
        took_fused = fn.fused is not None and fused_sampler_kind(self.sampler) is not None
        if not took_fused and self.clamp:            # the fused loop applies the final clamp itself (mdt_clamp)
            x = x.clamp(-1.0, 1.0)
        return x


class DiffusionInpainter(nn.Module):
    """diffusion.py:594-625."""

    def __init__(self, diffusion, *, num_steps: int, num_resamples: int, sampler: Sampler, sigma_schedule):
        super().__init__()
        self.denoise_fn = diffusion.denoise_fn
        self.num_steps = num_steps
        self.num_resamples = num_resamples
        self.inpaint_fn = sampler.inpaint
        self.sigma_schedule = sigma_schedule

    @torch.no_grad()
    def forward(self, inpaint: Tensor, inpaint_mask: Tensor, *, draw=None, seed=None, sample0: int = 0, tokens=None,
                **kwargs) -> Tensor:
        """``inpaint`` / ``inpaint_mask``: the dense fp32 (B, C, L) source and its bool mask, as in the reference -- or, on the
        fused path only, integer (B, L) draft ids and the bool (B, L) keep mask (run_adpm2_inpaint's token form).  ``tokens``
        (B, L) int32: receives the decode of the result (fused path)."""
        fn = BoundDenoise(self.denoise_fn, kwargs, dict(draw=draw, seed=seed, sample0=sample0, tokens=tokens))
        return self.inpaint_fn(source=inpaint, mask=inpaint_mask, fn=fn, sigmas=self.sigma_schedule(self.num_steps, inpaint.device),
                               num_steps=self.num_steps, num_resamples=self.num_resamples)


# ----------------------------------------------------------------------------------------------
# the fused sampling loop
# ----------------------------------------------------------------------------------------------
def _f32(t: Tensor, device) -> Tensor:
    return t.to(device=device, dtype=torch.float32).contiguous()


def guidance_rows(cond_scale, B: int, name: str = "cond_scale") -> Union[float, Tensor]:
    """The guidance scale of a call in the form the fused loops take: a float -- ONE scale for the batch, today's path -- or an
    fp32 CPU tensor of B values, one per sample (mdt_cfg_mix_rows).

    A Python number or a 0-dim tensor / array gives the float.  A 1-D list, tuple, ndarray or tensor of exactly B finite values
    gives the tensor -- or, when all its values are equal, that value as a float: the call is then literally the scalar call.
    Anything else raises ValueError naming the argument (``name``).  Sample b at scale 1 is not guided, as in the reference
    (modules.py:1248): it keeps its conditional prediction bit for bit."""
    def refuse(why):
        return ValueError(f"{name} must be a number or hold one finite value per sample ({B}): {why}")
    if isinstance(cond_scale, (bool, complex)):
        raise refuse(f"got a {type(cond_scale).__name__}")
    if isinstance(cond_scale, (int, float)):
        if not math.isfinite(cond_scale):
            raise refuse(f"got {cond_scale}")
        return float(cond_scale)
    try:
        t = torch.as_tensor(cond_scale)
    except Exception as e:
        raise refuse(f"got {type(cond_scale).__name__} ({e})") from None
    if t.dtype == torch.bool or t.is_complex():
        raise refuse(f"got dtype {t.dtype}")
    if t.dim() > 1:
        raise refuse(f"got {t.dim()} dimensions, shape {tuple(t.shape)}")
    if t.dim() == 0:
        return guidance_rows(t.item(), B, name)
    # rounded to fp32 once, here: the kernels take the scale as a float
    t = t.detach().to(device="cpu", dtype=torch.float32)
    if not bool(torch.isfinite(t).all()):
        raise refuse("got a NaN or an infinity")
    if t.numel() != B:
        raise refuse(f"got {t.numel()} values")
    if B == 0:
        return 1.0                                   # an empty batch: nothing to guide
    if bool((t == t[0]).all()):
        return float(t[0])
    return t.contiguous().clone()


def is_guided(scale) -> bool:
    """Whether a normalised guidance scale (guidance_rows) asks for the unconditional pass: a float != 1, or a tensor."""
    return isinstance(scale, torch.Tensor) or scale != 1.0


def scalar_guidance(scale, what: str) -> float:
    """The scale for a per-step seam (a caller's fn, a sampler with its own step(), denoise_fn / net() called directly): these
    evaluate the network with ONE scale."""
    if isinstance(scale, (list, tuple)) or getattr(scale, "ndim", 0) > 0:
        raise TypeError(f"{what}: a per-sample guidance scale needs the fused loop (sample() / inpaint() with ADPM2Sampler, "
                        "AEulerSampler or KarrasSampler); this seam takes one scale per call")
    return float(scale)


def _guided_setup(engine, embedding: Tensor, guided: bool) -> bool:
    """reserve() + prepare_context() for a sampling run.  Guidance runs both passes of UNetCFG1d.forward
    (modules.py:1248-1253) as ONE evaluation of the doubled batch [samples | samples] when the engine has that program
    (every cross-attention block on a ring kernel) and no cross-attention workgroup would straddle the halves (B a
    multiple of the samples per workgroup, CompiledUNet.dual_multiple); otherwise two passes.
    Returns whether the doubled batch is in use."""
    B = embedding.shape[0]
    dual = guided and engine.has_dual and B > 0 and B % engine.c.dual_multiple == 0
    engine.reserve(2 * B if dual else B)
    engine.prepare_context(torch.cat([embedding, embedding]) if dual else embedding)
    return dual


def _guided_eval(engine, lib, B: int, guided: bool, dual: bool, embedding_scale, st) -> Tensor:
    """net(x, t, embedding, embedding_scale) of engine.xin[:B] -> prediction rows [:B] (UNetCFG1d.forward).  ``embedding_scale``:
    a float, or the (B,) fp32 DEVICE tensor of one scale per sample (mdt_cfg_mix_rows)."""
    if dual:
        engine.xin[B:].copy_(engine.xin[:B], non_blocking=True)
        both = engine.eval(dual=True)
        pred, um = both[:B], both[B:]
    else:
        pred = engine.eval(False)
        um = engine.eval(True) if guided else None
    if guided and isinstance(embedding_scale, torch.Tensor):
        rt.check(lib.mdt_cfg_mix_rows(rt.ptr(pred), rt.ptr(um), rt.ptr(pred), rt.ptr(embedding_scale), B, pred.numel() // B, st))
    elif guided:
        rt.check(lib.mdt_cfg_mix(rt.ptr(pred), rt.ptr(um), rt.ptr(pred), float(embedding_scale), pred.numel(), st))
    return pred


class _Loop:
    """The scaffold every fused loop runs on: context and time table, the state initialised from the first draw, the draws in
    call order, the timed guided evaluation, the per-sample dynamic threshold, the step trace, final clamp and decode.

    ``explicit(k)`` returns the caller's tensor for draw k of the call (0 = the initial draw) or None: that draw then comes
    from the counter-based generator keyed by (seed, k, sample0 + b).  ``embedding_scale``: whatever guidance_rows takes -- one
    scale, or one per sample.

    ``first`` / ``hook``: the step functions run steps ``first .. len(steps) - 1`` of the plan and call ``hook(i, x)`` in front of
    step i, x being the state that step reads.  Without a hook the state is the scaled first draw, as every sampler's forward()
    starts; with one (run_refine) it starts zero-filled, the hook fills it, and the draws of the steps keep their absolute index
    (step i takes draw i + 1), so draw 0 is left to the hook."""

    def __init__(self, engine, embedding, shape, sigmas, steps, explicit, seed, sample0, embedding_scale, dynamic_threshold,
                 clamp=False, trace=None, timer=None, tokens=None, first=0, hook=None):
        self.lib, self.engine = rt.load_library(), engine
        (self.B, self.C, self.L), self.Cp = shape, engine.c.in_pad
        self.explicit, self.seed, self.sample0, self.draws = explicit, seed or 0, sample0, 0
        scale = guidance_rows(embedding_scale, self.B, "embedding_scale")
        self.guided, self.q = is_guided(scale), float(dynamic_threshold)
        # one scale per sample: uploaded once per call, read by mdt_cfg_mix_rows after every evaluation
        self.scale = scale.to(engine.device) if isinstance(scale, torch.Tensor) else scale
        self.clamp, self.trace, self.timer, self.tokens = clamp, trace, timer, tokens
        self.st = rt.current_stream()
        engine.handoff_check()                        # a time-out of the previous call's pair hand-offs is reported here
        self.dual = _guided_setup(engine, embedding, self.guided)
        engine.prepare_times(torch.tensor(plan_time_rows(steps), dtype=torch.float32))
        self.first, self.hook = first, hook
        self.dscale = torch.empty(self.B, device=engine.device) if dynamic_threshold else None   # clip()'s dynamic threshold
        if hook is not None:
            self.x, self.draws = torch.zeros(self.B, self.C, self.L, device=engine.device), first + 1
            engine.xin[:self.B].zero_()               # a row that has not started yet rides along on zeros
            return
        self.x = torch.empty(self.B, self.C, self.L, device=engine.device)
        nz, k = self.draw()
        rt.check(self.lib.mdt_init_noise(rt.ptr(self.x), rt.ptr(nz), float(sigmas[0]), self.seed, k, self.sample0,
                                         self.B, self.C, self.L, self.st))

    def dims(self):
        return self.B, self.C, self.L, self.Cp

    def draw(self):
        """The next draw of the call: (the explicit tensor on the device or None, its index for the generator)."""
        k, self.draws = self.draws, self.draws + 1
        nz = self.explicit(k)
        return (None if nz is None else _f32(nz, self.engine.device)), k

    def enter(self, i: int, x: Tensor) -> None:
        if self.hook is not None:
            self.hook(i, x)

    def dyn(self, xs: Tensor, pred: Tensor, w: ScaleWeights) -> int:
        if self.dscale is not None:
            rt.check(self.lib.mdt_dyn_scale(rt.ptr(xs), rt.ptr(pred), rt.ptr(self.dscale), w.c_skip, w.c_out, self.q,
                                            self.B, self.C, self.L, self.Cp, self.st))
        return rt.ptr(self.dscale)

    def unet(self, row: int) -> Tensor:
        self.engine.select_time(row)
        if self.timer is not None:
            self.timer.start()
        pred = _guided_eval(self.engine, self.lib, self.B, self.guided, self.dual, self.scale, self.st)
        if self.timer is not None:
            self.timer.stop()
        return pred

    def tok(self, last: bool) -> int:
        """``tokens`` for the last update kernel (it decodes what it writes) -- unless the final clamp comes first."""
        return rt.ptr(self.tokens) if (last and not self.clamp) else 0

    def record(self, i: int, x: Tensor) -> None:
        if self.trace is not None and (i + 1) in self.trace.get("want", ()):
            self.trace[i + 1] = x.clone()

    def finish(self, x: Tensor, decoded: bool, handoff: bool = True) -> Tensor:
        """Final clamp (mdt_clamp) and the decode when the last update kernel has not done it."""
        if self.clamp:
            rt.check(self.lib.mdt_clamp(rt.ptr(x), -1.0, 1.0, x.numel(), self.st))
        if self.tokens is not None and (self.clamp or not decoded):   # clamping creates ties (first maximum wins): decode after it
            rt.check(self.lib.mdt_argmax_tokens(rt.ptr(x), rt.ptr(self.tokens), self.B, self.C, self.L, self.st))
        if handoff:
            self.engine.note_handoff()
        return x


def _adpm2_step(lp: _Loop, i: int, s: StepScalars, x_mid: Tensor, c_in_next: Optional[float], tok: int) -> None:
    """ADPM2Sampler.step (diffusion.py:502-515) on lp.x, whose scaled copy is in engine.xin: evaluation at sigma,
    mdt_adpm2_mid, evaluation at sigma_mid, the step's draw, mdt_adpm2_next.  ``c_in_next``: the input scale of the NEXT
    evaluation, which mdt_adpm2_next then prepares in engine.xin (None: it does not)."""
    lib, x, xin, st = lp.lib, lp.x, lp.engine.xin, lp.st
    pred = lp.unet(2 * i)
    rt.check(lib.mdt_adpm2_mid(rt.ptr(x), rt.ptr(pred), rt.ptr(x_mid), rt.ptr(xin), s.w.c_skip, s.w.c_out, s.sigma, s.dt_mid,
                               s.w_mid.c_in, *lp.dims(), lp.dyn(x, pred, s.w), st))
    pred = lp.unet(2 * i + 1)
    nz, k = lp.draw()
    rt.check(lib.mdt_adpm2_next(rt.ptr(x), rt.ptr(x_mid), rt.ptr(pred), rt.ptr(nz), 0 if c_in_next is None else rt.ptr(xin),
                                s.w_mid.c_skip, s.w_mid.c_out, s.sigma_mid, s.dt_down, s.sigma_up,
                                0.0 if c_in_next is None else c_in_next, lp.seed, k, lp.sample0, *lp.dims(), tok,
                                lp.dyn(x_mid, pred, s.w_mid), st))


def _adpm2_steps(lp: _Loop, steps) -> Tensor:
    """ADPM2Sampler.forward (diffusion.py:517-524): two evaluations per step."""
    x_mid = torch.empty_like(lp.x)
    if lp.hook is None:
        rt.check(lp.lib.mdt_precond_in(rt.ptr(lp.x), rt.ptr(lp.engine.xin), steps[0].w.c_in, *lp.dims(), lp.st))
    for i in range(lp.first, len(steps)):
        s, last = steps[i], i + 1 == len(steps)
        lp.enter(i, lp.x)
        _adpm2_step(lp, i, s, x_mid, None if last else steps[i + 1].w.c_in, lp.tok(last))
        lp.record(i, lp.x)
    return lp.x


def _aeuler_steps(lp: _Loop, steps) -> Tensor:
    """AEulerSampler.forward (diffusion.py:476-483): one evaluation and one mdt_aeuler_next launch per step."""
    lib, x, xin, st = lp.lib, lp.x, lp.engine.xin, lp.st
    if lp.hook is None:
        rt.check(lib.mdt_precond_in(rt.ptr(x), rt.ptr(xin), steps[0].w.c_in, *lp.dims(), st))
    for i in range(lp.first, len(steps)):
        s = steps[i]
        lp.enter(i, x)
        pred = lp.unet(i)
        nz, k = lp.draw()
        last = i + 1 == len(steps)
        c_in_next = 0.0 if last else steps[i + 1].w.c_in
        rt.check(lib.mdt_aeuler_next(rt.ptr(x), rt.ptr(pred), rt.ptr(nz), 0 if last else rt.ptr(xin), s.w.c_skip, s.w.c_out,
                                     s.sigma, s.dt, s.sigma_up, c_in_next, lp.seed, k, lp.sample0, *lp.dims(), lp.tok(last),
                                     lp.dyn(x, pred, s.w), st))
        lp.record(i, x)
    return x


def _karras_steps(lp: _Loop, steps) -> Tensor:
    """KarrasSampler.forward (diffusion.py:437-453).  Per step: the draw, mdt_karras_hat (churn; in place on x), evaluation at
    sigma_hat, mdt_karras_mid, evaluation at sigma_next, mdt_karras_next."""
    lib, x, xin, st = lp.lib, lp.x, lp.engine.xin, lp.st
    d, x_next = torch.empty_like(x), torch.empty_like(x)
    for i in range(lp.first, len(steps)):
        s = steps[i]
        lp.enter(i, x)
        nz, k = lp.draw()
        rt.check(lib.mdt_karras_hat(rt.ptr(x), rt.ptr(nz), rt.ptr(x), rt.ptr(xin), s.noise_scale, s.s_noise, s.w_hat.c_in,
                                    lp.seed, k, lp.sample0, *lp.dims(), st))                        # x is x_hat from here
        pred = lp.unet(s.row_hat)
        tok = lp.tok(i + 1 == len(steps))
        if s.euler_only:
            rt.check(lib.mdt_karras_mid(rt.ptr(x), rt.ptr(pred), rt.ptr(d), rt.ptr(x_next), 0, s.w_hat.c_skip, s.w_hat.c_out,
                                        s.sigma_hat, s.dt, 0.0, *lp.dims(), tok, lp.dyn(x, pred, s.w_hat), st))
            x, x_next = x_next, x
        else:
            rt.check(lib.mdt_karras_mid(rt.ptr(x), rt.ptr(pred), rt.ptr(d), rt.ptr(x_next), rt.ptr(xin), s.w_hat.c_skip,
                                        s.w_hat.c_out, s.sigma_hat, s.dt, s.w_next.c_in, *lp.dims(), 0,
                                        lp.dyn(x, pred, s.w_hat), st))
            pred = lp.unet(s.row_next)
            rt.check(lib.mdt_karras_next(rt.ptr(x), rt.ptr(x_next), rt.ptr(d), rt.ptr(pred), rt.ptr(x), s.w_next.c_skip,
                                         s.w_next.c_out, s.sigma_next, s.half, *lp.dims(), tok,
                                         lp.dyn(x_next, pred, s.w_next), st))
        lp.record(i, x)
    return x


class FusedKind(NamedTuple):
    cls: type           # the sampler class; a subclass without a step() of its own takes the same loop
    params: tuple       # its constructor parameters: sampler_params of mdt::sample_with, in this order
    plan: Callable      # (num_steps, schedule, sampler, sigma_data) -> (sigmas, per-step scalars)
    steps: Callable     # (_Loop, per-step scalars) -> the final state


# kind -> everything that differs between the fused loops; a kind's position is its sampler_kind in mdt::sample_with
FUSED_SAMPLERS = {"adpm2": FusedKind(ADPM2Sampler, ("rho",), adpm2_plan, _adpm2_steps),
                  "aeuler": FusedKind(AEulerSampler, (), aeuler_plan, _aeuler_steps),
                  "karras": FusedKind(KarrasSampler, ("s_tmin", "s_tmax", "s_churn", "s_noise"), karras_plan, _karras_steps)}


def require_fused_kind(sampler) -> str:
    kind = fused_sampler_kind(sampler)
    if kind is None:
        raise TypeError(f"{type(sampler).__name__} has no fused loop")
    return kind


def run_sampler(engine, embedding: Tensor, pred_dim: int, num_steps: int, noise: NoiseSource, schedule, sampler: Sampler,
                sigma_data: float, embedding_scale=1.0, clamp: bool = False, trace: Optional[dict] = None, timer=None,
                tokens: Optional[Tensor] = None, dynamic_threshold: float = 0.0) -> Tensor:
    """DiffusionSampler.forward (diffusion.py:577-591) + the sampler's forward() + KDiffusion_mod.denoise_fn (:798-814) +
    UNetCFG1d.forward (modules.py:1228-1255) on the GPU, for any sampler with a fused kind.
    ``tokens`` (B, L) int32: also the decode step after the path, argmax over channels of the final sample
    (generative.py:1212-1213), written by the last update kernel.  ``embedding_scale``: one guidance scale, or one per sample
    (guidance_rows): row b is then the row of the call at scale[b], bit for bit under one kernel_choice."""
    kind = FUSED_SAMPLERS[require_fused_kind(sampler)]
    sigmas, steps = kind.plan(num_steps, schedule, sampler, sigma_data)

    def explicit(k: int):            # every sampler draws once per step: draw 0 is the initial one, draw i + 1 that of step i
        if k == 0:
            return noise.init
        return None if noise.steps is None else noise.steps(k - 1)
    with torch.cuda.device(engine.device):
        lp = _Loop(engine, embedding, (embedding.shape[0], pred_dim, engine.c.length), sigmas, steps, explicit, noise.seed,
                   noise.sample0, embedding_scale, dynamic_threshold, clamp, trace, timer, tokens)
        if steps:
            return lp.finish(kind.steps(lp, steps), decoded=True)
        # num_steps == 1: the clamped first draw, decoded; nothing was evaluated, so there is no hand-off to note.  The ADPM2
        # loop has always clamped it with Tensor.clamp, which keeps a NaN (KarrasSchedule(num_steps=1) is 0 / 0) where
        # mdt_clamp returns -1; each sampler keeps what it did
        if clamp and kind.cls is ADPM2Sampler:
            lp.x, lp.clamp = lp.x.clamp(-1.0, 1.0), False
        return lp.finish(lp.x, decoded=False, handoff=False)


def run_adpm2_inpaint(engine, embedding: Tensor, source: Tensor, mask: Tensor, num_steps: int, num_resamples: int,
                      draw: Optional[Callable[[], Tensor]], seed: Optional[int], schedule,
                      sampler: ADPM2Sampler, sigma_data: float, embedding_scale=1.0,
                      sample0: int = 0, dynamic_threshold: float = 0.0, *, draft: Optional[Tensor] = None,
                      keep: Optional[Tensor] = None, pred_dim: Optional[int] = None, tokens: Optional[Tensor] = None) -> Tensor:
    """ADPM2Sampler.inpaint (diffusion.py:526-549) behind DiffusionInpainter.forward (:612-625).
    ``draw()`` returns the next torch.randn_like tensor in the reference's call order (parity mode);
    otherwise draws come from the counter-based generator keyed by (seed, draw index).

    The source comes dense -- ``source`` fp32 (B, C, L) with the bool ``mask`` of its shape -- or, with ``source`` and ``mask``
    None, as token ids: ``draft`` integer (B, L) standing for its +-1 one-hot over ``pred_dim`` channels and ``keep`` bool
    (B, L), the mask before its repeat over the channels (generative.py:1600-1603).  Both forms run the same loop on
    mdt_inpaint_enter / mdt_inpaint_finish.  ``tokens`` (B, L) int32: also the decode of the result (argmax over channels; with a
    draft, the draft id at a kept position), written by mdt_inpaint_finish.  ``embedding_scale`` as run_sampler."""
    sigmas, steps = adpm2_plan(num_steps, schedule, sampler, sigma_data)
    dev = engine.device
    if source is not None:
        if draft is not None or keep is not None:
            raise ValueError("give the source either dense (source, mask) or as token ids (draft, keep)")
        if mask.dtype != torch.bool or tuple(mask.shape) != tuple(source.shape):
            raise ValueError("in_paint_mask must be a bool tensor of the same shape as inpaint")
        shape, per_token, kp = tuple(source.shape), 0, mask
    else:
        if draft is None or keep is None or pred_dim is None:
            raise ValueError("the token form needs draft, keep and pred_dim")
        if draft.dim() != 2 or keep.dtype != torch.bool or tuple(keep.shape) != tuple(draft.shape):
            raise ValueError("draft must be (B, L) token ids and keep a bool tensor of the same shape")
        shape, per_token, kp = (draft.shape[0], int(pred_dim), draft.shape[1]), 1, keep
    with torch.cuda.device(dev):
        lp = _Loop(engine, embedding, shape, sigmas, steps, lambda k: None if draw is None else draw(), seed,
                   sample0, embedding_scale, dynamic_threshold)
        lib, x, st = lp.lib, lp.x, lp.st
        B, C, L, Cp = lp.dims()
        src = None if source is None else _f32(source, dev)
        ids = None if draft is None else draft.to(device=dev, dtype=torch.int32).contiguous()
        mk = kp.to(device=dev).to(torch.uint8).contiguous()
        x_mid = torch.empty_like(x)
        for i, s in enumerate(steps):
            src_nz, src_k = lp.draw()                     # source_noisy = source + sigmas[i] * randn_like(source)
            re_nz, re_k, renoise = None, 0, 0.0           # the re-noise of the previous resample: applied on entry to the next
            for r in range(num_resamples):
                rt.check(lib.mdt_inpaint_enter(rt.ptr(x), rt.ptr(engine.xin), rt.ptr(src), rt.ptr(ids), rt.ptr(mk), per_token,
                                               rt.ptr(src_nz), rt.ptr(re_nz), s.sigma, renoise, s.w.c_in, lp.seed, src_k, re_k,
                                               sample0, B, C, L, Cp, st))
                _adpm2_step(lp, i, s, x_mid, None, 0)
                if r < num_resamples - 1:
                    (re_nz, re_k), renoise = lp.draw(), s.renoise
        rt.check(lib.mdt_inpaint_finish(rt.ptr(x), rt.ptr(src), rt.ptr(ids), rt.ptr(mk), per_token, rt.ptr(tokens), B, C, L, st))
        return lp.finish(x, decoded=True)


# ----------------------------------------------------------------------------------------------
# refine: noise a source up to the level of step k and run the remaining steps, k per sample
# ----------------------------------------------------------------------------------------------
def refine_start(timesteps: int, strength):
    """The start step of a refine call for a ``strength`` in (0, 1], the share of the schedule that is run:
    ``steps_run = min(T - 1, max(1, ceil(strength * (T - 1))))`` and ``start = T - 1 - steps_run``.  Strength 1 is start 0 (all
    T - 1 steps from the highest noise level: far-away results), a small strength the last step alone (near ones).  ``strength``
    may be a 1-D sequence, one entry per sample: the result is then a list of ints."""
    if isinstance(timesteps, bool) or not isinstance(timesteps, int) or timesteps < 2:
        raise ValueError(f"timesteps must be an int >= 2 (a refine call runs at least one step), got {timesteps!r}")

    def one(v) -> int:
        if isinstance(v, (bool, complex)) or not isinstance(v, (int, float)) or not (0.0 < v <= 1.0):
            raise ValueError(f"strength must lie in (0, 1], got {v!r}")
        return timesteps - 1 - min(timesteps - 1, max(1, math.ceil(v * (timesteps - 1))))
    if isinstance(strength, (bool, int, float, complex)):
        return one(strength)
    try:
        t = torch.as_tensor(strength)
    except Exception as e:
        raise ValueError(f"strength must be a number in (0, 1] or a 1-D sequence of them ({e})") from None
    if t.dim() == 0:
        return one(t.item())
    if t.dim() != 1 or t.dtype == torch.bool or t.is_complex():
        raise ValueError(f"strength must be a number in (0, 1] or a 1-D sequence of them, got shape {tuple(t.shape)} {t.dtype}")
    return [one(v) for v in t.double().tolist()]


def start_rows(start_step, B: int, timesteps: int, name: str = "start_step") -> Union[int, Tensor]:
    """The start step of a refine call in the form run_refine takes: an int -- ONE start for the batch -- or an int32 CPU tensor
    of B values, one per sample.

    A Python int or a 0-dim integer tensor / array gives the int.  A 1-D list, tuple, ndarray or integer tensor of exactly B
    entries gives the tensor -- or, when all entries are equal, that entry as an int: the call is then literally the scalar call.
    Every entry lies in [0, timesteps - 2].  Anything else (a float, a bool, a wrong length, a value out of range) raises
    ValueError naming the argument (``name``)."""
    def refuse(why):
        return ValueError(f"{name} must be an int in [0, {timesteps - 2}] (timesteps - 2) or hold one per sample ({B}): {why}")
    if isinstance(timesteps, bool) or not isinstance(timesteps, int) or timesteps < 2:
        raise ValueError(f"timesteps must be an int >= 2 (a refine call runs at least one step), got {timesteps!r}")
    if isinstance(start_step, (bool, float, complex)) or start_step is None:
        raise refuse(f"got {start_step!r} ({type(start_step).__name__})")
    if isinstance(start_step, int):
        if not 0 <= start_step <= timesteps - 2:
            raise refuse(f"got {start_step}")
        return int(start_step)
    try:
        t = torch.as_tensor(start_step)
    except Exception as e:
        raise refuse(f"got {type(start_step).__name__} ({e})") from None
    if B == 0 and t.dim() == 1 and t.numel() == 0:
        return 0                                     # an empty batch: nothing to start (an empty list has no integer dtype)
    if t.dtype == torch.bool or t.is_floating_point() or t.is_complex():
        raise refuse(f"got dtype {t.dtype}")
    if t.dim() > 1:
        raise refuse(f"got {t.dim()} dimensions, shape {tuple(t.shape)}")
    t = t.detach().to(device="cpu", dtype=torch.int64)
    if t.dim() == 0:
        return start_rows(int(t), B, timesteps, name)
    if t.numel() != B:
        raise refuse(f"got {t.numel()} values")
    if int(t.min()) < 0 or int(t.max()) > timesteps - 2:
        raise refuse(f"got values in [{int(t.min())}, {int(t.max())}]")
    if bool((t == t[0]).all()):
        return int(t[0])
    return t.to(torch.int32).contiguous()


def run_refine(engine, embedding: Tensor, pred_dim: int, num_steps: int, noise: NoiseSource, schedule, sampler: Sampler,
               sigma_data: float, start, *, source: Optional[Tensor] = None, draft: Optional[Tensor] = None,
               embedding_scale=1.0, clamp: bool = False, trace: Optional[dict] = None, timer=None,
               tokens: Optional[Tensor] = None, dynamic_threshold: float = 0.0, keep: Optional[Tensor] = None,
               keep_per_token: bool = False) -> Tensor:
    """Partial-noise editing on the fused loop, for any sampler with a fused kind: row b is
    ``x = source + sigmas[k] * draw0`` (the expression of diffusion.py:535) followed by the sampler's unchanged step() for
    i = k .. num_steps - 2, with k = ``start`` (an int) or ``start[b]`` (int32, B entries; start_rows).

    The source comes dense -- ``source`` fp32 (B, C, L) -- or as ``draft`` integer ids (B, L) standing for their +-1 one-hot over
    ``pred_dim`` channels, the two source forms of run_adpm2_inpaint.  The plan and the time table are those of the full
    ``num_steps`` call, so a step keeps its scalars and its time row; steps min(start) .. num_steps - 2 run.  Draw 0 is the entry
    noise of every row whatever its start, step i takes draw i + 1 (run_sampler's index): a row's result depends on its own start
    only -- row b of a per-sample call is row b of the scalar call at start[b], bit for bit under one kernel_choice -- and
    ``noise.steps(i)`` is not called for i < min(start).  A row that has not started yet rides along, its state ignored, until
    mdt_refine_enter overwrites its state and network input in front of its step: a per-sample call costs every row the steps
    from min(start).  ``clamp`` / ``trace`` / ``timer`` / ``tokens`` / ``embedding_scale`` / ``dynamic_threshold`` as run_sampler.

    ``keep`` (bool, True = keep; (B, C, L), or (B, L) with ``keep_per_token``): refine around a kept scaffold.  In front of EVERY
    step i from min(start), mdt_refine_keep_enter sets the kept positions of the rows that run to ``source + sigmas[i] * n_src(i)``
    (the merge of ADPM2Sampler.inpaint, diffusion.py:539-542, as a select) and enters the rows whose start is i; after the last
    step mdt_inpaint_finish sets them to the source (:549) and decodes -- the last update kernel does not -- and the clamp comes
    after that merge.  There are no resamples.  The source draw of step i is draw ``num_steps + i`` of the generator, or
    ``noise.sources(i)`` next to explicit (init, steps) -- which is then required, and like steps(i) not called for
    i < min(start): the draws 0 and i + 1 stay what they are, so an all-False mask gives the unmasked call's result and a row
    still depends on its own start only.  Without ``keep`` the call launches exactly what it launched before the mask existed."""
    kind = FUSED_SAMPLERS[require_fused_kind(sampler)]
    sigmas, steps = kind.plan(num_steps, schedule, sampler, sigma_data)
    dev, B = engine.device, embedding.shape[0]
    if B == 0:
        raise ValueError("run_refine needs at least one sample (refine() returns the empty result itself)")
    start = start_rows(start, B, num_steps, "start")
    if (source is None) == (draft is None):
        raise ValueError("give the source either dense (source) or as token ids (draft)")
    shape = (B, int(pred_dim), engine.c.length)
    if source is not None and tuple(source.shape) != shape:
        raise ValueError(f"source is {tuple(source.shape)}, the call refines {shape}")
    if draft is not None and (draft.is_floating_point() or tuple(draft.shape) != (B, engine.c.length)):
        raise ValueError(f"draft must be integer token ids ({B}, {engine.c.length}), got {draft.dtype} {tuple(draft.shape)}")
    if noise.init is not None and tuple(noise.init.shape) != shape:
        raise ValueError(f"the entry noise is {tuple(noise.init.shape)}, the call refines {shape}")
    if keep is not None:
        want = (B, engine.c.length) if keep_per_token else shape
        if keep.dtype != torch.bool or tuple(keep.shape) != want:
            raise ValueError(f"keep must be a bool tensor {want}, got {keep.dtype} {tuple(keep.shape)}")
        if noise.steps is not None and noise.sources is None:
            raise ValueError("a refine call with a keep mask and explicit (init, steps) noise needs NoiseSource(sources=...): the "
                             "draw that noises the kept source in front of step i")
    rows = start if isinstance(start, torch.Tensor) else torch.full((B,), start, dtype=torch.int32)
    entries = set(rows.tolist())

    def explicit(k: int):            # run_sampler's draws: 0 is the entry noise, i + 1 that of step i
        if k == 0:
            return noise.init
        return None if noise.steps is None else noise.steps(k - 1)
    with torch.cuda.device(dev):
        src = None if source is None else _f32(source, dev)
        ids = None if draft is None else draft.to(device=dev, dtype=torch.int32).contiguous()
        nz0 = None if noise.init is None else _f32(noise.init, dev)
        start_dev = rows.to(dev)

        def enter(i: int, x: Tensor) -> None:
            if i in entries:
                s = steps[i]
                c_in = (s.w_hat if isinstance(s, KarrasStep) else s.w).c_in
                rt.check(lp.lib.mdt_refine_enter(rt.ptr(x), rt.ptr(engine.xin), rt.ptr(start_dev), i, rt.ptr(src), rt.ptr(ids),
                                                 rt.ptr(nz0), float(sigmas[i]), c_in, lp.seed, 0, lp.sample0, *lp.dims(), lp.st))
        if keep is None:
            lp = _Loop(engine, embedding, shape, sigmas, steps, explicit, noise.seed, noise.sample0, embedding_scale,
                       dynamic_threshold, clamp, trace, timer, tokens, first=min(entries), hook=enter)
            return lp.finish(kind.steps(lp, steps), decoded=True)
        mk, per_token = keep.to(device=dev).to(torch.uint8).contiguous(), 1 if keep_per_token else 0

        def enter_keep(i: int, x: Tensor) -> None:
            s = steps[i]
            c_in = (s.w_hat if isinstance(s, KarrasStep) else s.w).c_in
            nsrc = None if noise.steps is None else _f32(noise.sources(i), dev)
            rt.check(lp.lib.mdt_refine_keep_enter(rt.ptr(x), rt.ptr(engine.xin), rt.ptr(start_dev), i, rt.ptr(src), rt.ptr(ids),
                                                  rt.ptr(mk), per_token, rt.ptr(nz0), rt.ptr(nsrc), float(sigmas[i]), c_in, lp.seed,
                                                  0, num_steps + i, lp.sample0, *lp.dims(), lp.st))
        # the loop decodes nothing (tokens=None): mdt_inpaint_finish merges and decodes, then finish() clamps and decodes again
        lp = _Loop(engine, embedding, shape, sigmas, steps, explicit, noise.seed, noise.sample0, embedding_scale,
                   dynamic_threshold, clamp, trace, timer, None, first=min(entries), hook=enter_keep)
        x = kind.steps(lp, steps)
        rt.check(lp.lib.mdt_inpaint_finish(rt.ptr(x), rt.ptr(src), rt.ptr(ids), rt.ptr(mk), per_token, rt.ptr(tokens), *shape, lp.st))
        lp.tokens = tokens
        return lp.finish(x, decoded=True)
