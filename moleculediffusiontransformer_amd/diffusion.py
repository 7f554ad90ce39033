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
from typing import Callable, List, Optional, Sequence

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


class ADPM2Sampler(Sampler):
    """diffusion.py:486-549: second-order ancestral DPM-2 sampler.

    ``fn(x, sigma=...)`` is any denoiser on HIP tensors.  When it is the denoiser of a QMDiffusion* model (the closure
    DiffusionSampler / DiffusionInpainter build), forward()/inpaint() run the whole loop on the fused path (run_adpm2:
    per-step scalars precomputed on the host, preconditioning + update fused, the U-Net as a replayed HIP graph); with any
    other ``fn`` every step is two calls of ``fn`` and two mdt_adpm2_euler launches (the reference's arithmetic, fp32, no
    contraction), drawing the step noise with torch.randn_like on the device exactly as diffusion.py:514 does."""

    diffusion_types = [_KAlias("k"), _KAlias("vk")]

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
        sigma = torch.as_tensor(sigma, dtype=torch.float32).cpu().reshape(())
        sigma_next = torch.as_tensor(sigma_next, dtype=torch.float32).cpu().reshape(())
        sigma_up, sigma_down, sigma_mid = self.get_sigmas(sigma, sigma_next)
        dt_mid, dt_down = float(sigma_mid - sigma), float(sigma_down - sigma)     # fp32 tensor arithmetic, as the reference
        up32 = float(torch.tensor(sigma_up, dtype=torch.float32))
        if x.device.type != "cuda":
            raise RuntimeError("ADPM2Sampler.step runs on an AMD GPU through libmdt_hip.so (no CPU fallback)")
        x = x.detach().float().contiguous()
        B, C, L = x.shape
        with torch.no_grad(), torch.cuda.device(x.device):
            st = rt.current_stream()
            den = fn(x, sigma=sigma).float().contiguous()
            x_mid = torch.empty_like(x)
            rt.check(lib.mdt_adpm2_euler(rt.ptr(x), rt.ptr(x), rt.ptr(den), 0, rt.ptr(x_mid), float(sigma), dt_mid, 0.0, 0,
                                         0, 0, 0, B, C, L, st))
            den_mid = fn(x_mid, sigma=torch.as_tensor(sigma_mid, dtype=torch.float32)).float().contiguous()
            nz = (torch.randn_like(x) if noise is None else noise.to(device=x.device, dtype=torch.float32)).contiguous()
            out = torch.empty_like(x)
            rt.check(lib.mdt_adpm2_euler(rt.ptr(x), rt.ptr(x_mid), rt.ptr(den_mid), rt.ptr(nz), rt.ptr(out),
                                         float(sigma_mid), dt_down, up32, 1, 0, 0, 0, B, C, L, st))
        return out

    def forward(self, noise, fn: Callable, sigmas: Tensor, num_steps: int) -> Tensor:
        """diffusion.py:517-524.  ``noise`` is the initial draw (B, C, L) or, on the fused path, a NoiseSource."""
        fused = getattr(fn, "fused", None) if type(self).step is ADPM2Sampler.step else None   # a subclass's step() is honoured
        if fused is not None:
            return fused.sample(noise, self, sigmas, num_steps)
        if isinstance(noise, NoiseSource):
            raise TypeError("a NoiseSource drives the fused path only; pass the initial noise tensor with a custom fn")
        x = float(sigmas[0]) * noise
        for i in range(num_steps - 1):
            x = self.step(x, fn=fn, sigma=sigmas[i], sigma_next=sigmas[i + 1])
        return x

    def inpaint(self, source: Tensor, mask: Tensor, fn: Callable, sigmas: Tensor, num_steps: int,
                num_resamples: int) -> Tensor:
        """diffusion.py:526-549."""
        fused = getattr(fn, "fused", None) if type(self).step is ADPM2Sampler.step else None
        if fused is not None:
            return fused.inpaint(source, mask, self, sigmas, num_steps, num_resamples)
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


def _step_inputs(name: str, x: Tensor, sigma, sigma_next):
    """What every per-step path starts from: the two sigmas as 0-dim fp32 CPU tensors (the reference indexes a CPU schedule)
    and the state as a contiguous fp32 HIP tensor."""
    if x.device.type != "cuda":
        raise RuntimeError(f"{name}.step runs on an AMD GPU through libmdt_hip.so (no CPU fallback)")
    sigma = torch.as_tensor(sigma, dtype=torch.float32).cpu().reshape(())
    sigma_next = torch.as_tensor(sigma_next, dtype=torch.float32).cpu().reshape(())
    return x.detach().float().contiguous(), sigma, sigma_next


class AEulerSampler(Sampler):
    """diffusion.py:456-483: ancestral Euler sampler, ONE evaluation per step (ADPM2 and Karras take two).

    Same seams as ADPM2Sampler: with the denoiser of a QMDiffusion* model forward() runs the whole loop on the fused path
    (run_aeuler: one mdt_aeuler_next launch per step around the replayed U-Net graph); with any other ``fn`` every step is
    one call of ``fn`` and one mdt_adpm2_euler launch.  inpaint() is the base class's NotImplementedError, as in the
    reference."""

    diffusion_types = [_KAlias("k"), _KAlias("vk")]

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
            nz = (torch.randn_like(x) if noise is None else noise.to(device=x.device, dtype=torch.float32)).contiguous()
            out = torch.empty_like(x)
            rt.check(lib.mdt_adpm2_euler(rt.ptr(x), rt.ptr(x), rt.ptr(den), rt.ptr(nz), rt.ptr(out), float(sigma), dt, up32, 1,
                                         0, 0, 0, B, C, L, rt.current_stream()))
        return out

    def forward(self, noise, fn: Callable, sigmas: Tensor, num_steps: int) -> Tensor:
        """diffusion.py:476-483.  ``noise`` is the initial draw (B, C, L) or, on the fused path, a NoiseSource."""
        fused = getattr(fn, "fused", None) if fused_sampler_kind(self) else None          # a subclass's step() is honoured
        if fused is not None:
            return fused.sample(noise, self, sigmas, num_steps)
        if isinstance(noise, NoiseSource):
            raise TypeError("a NoiseSource drives the fused path only; pass the initial noise tensor with a custom fn")
        x = float(sigmas[0]) * noise
        for i in range(num_steps - 1):
            x = self.step(x, fn=fn, sigma=sigmas[i], sigma_next=sigmas[i + 1])
        return x


class KarrasSampler(Sampler):
    """diffusion.py:399-453: the stochastic second-order sampler of Karras et al. (arXiv:2206.00364, algorithm 2) AS THE
    REFERENCE WRITES IT.  Its correction line is ``x_next = x_hat + 0.5 * (sigma - sigma_hat) * (d + d_prime)`` (:434), not
    the paper's ``x_hat + 0.5 * (sigma_next - sigma_hat) * (d + d_prime)``: without churn (gamma = 0, the constructor's
    default) sigma_hat == sigma and every step returns x_hat = x, so ``KarrasSampler()`` returns ``sigmas[0] * noise`` bit
    for bit; with churn a step moves x by ``-0.5 gamma sigma (d + d')`` only.  This package reproduces the reference's
    arithmetic, so it does the same (pinned by tests/golden/tiny_b3_t8_karras0_sample.npz); it is not "fixed" here.

    With the denoiser of a QMDiffusion* model forward() runs the fused loop (run_karras: mdt_karras_hat / _mid / _next around
    the two evaluations of a step); with any other ``fn`` a step is two calls of ``fn`` plus elementwise launches."""

    diffusion_types = [_KAlias("k"), _KAlias("vk")]

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
            nz = (torch.randn_like(x) if noise is None else noise.to(device=x.device, dtype=torch.float32)).contiguous()
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

    def forward(self, noise, fn: Callable, sigmas: Tensor, num_steps: int) -> Tensor:
        """diffusion.py:437-453.  ``noise`` is the initial draw (B, C, L) or, on the fused path, a NoiseSource."""
        fused = getattr(fn, "fused", None) if fused_sampler_kind(self) else None          # a subclass's step() is honoured
        if fused is not None:
            return fused.sample(noise, self, sigmas, num_steps)
        if isinstance(noise, NoiseSource):
            raise TypeError("a NoiseSource drives the fused path only; pass the initial noise tensor with a custom fn")
        x = float(sigmas[0]) * noise
        sigmas = torch.as_tensor(sigmas, dtype=torch.float32).cpu()
        gammas = self.get_gammas(sigmas, num_steps)
        for i in range(num_steps - 1):
            x = self.step(x, fn=fn, sigma=sigmas[i], sigma_next=sigmas[i + 1], gamma=gammas[i])
        return x


def fused_sampler_kind(sampler) -> Optional[str]:
    """'adpm2' | 'aeuler' | 'karras' when ``sampler`` may take the fused loop of a QMDiffusion* model -- one of the three
    sampler classes with its own step() (a subclass that overrides step() is honoured: it gets the per-step path) -- else None."""
    for kind, cls in (("adpm2", ADPM2Sampler), ("aeuler", AEulerSampler), ("karras", KarrasSampler)):
        if isinstance(sampler, cls):
            return kind if type(sampler).step is cls.step else None
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


def adpm2_plan(num_steps: int, schedule, sampler: ADPM2Sampler, sigma_data: float):
    """Per-step scalars of ADPM2Sampler.forward/step (diffusion.py:502-524), bit-for-bit as the reference
    computes them on CPU.  ``schedule`` is a KarrasSchedule or an already evaluated (num_steps + 1,) sigma tensor."""
    sigmas = schedule.detach().float().cpu() if isinstance(schedule, torch.Tensor) else schedule(num_steps)
    # The plan is a pure function of (sigmas, sampler, sigma_data) and costs ~10 ms of 0-dim tensor arithmetic for 64 timesteps
    # (it has to: the reference's mixed double / fp32 rounding is reproduced op by op).  Hidden while the GPU queue is full, but a
    # call that waits for its hand-off status (engine.note_handoff) exposes the NEXT call's host prologue: keep the last plans.
    key = (num_steps, sigmas.numpy().tobytes(), type(sampler), float(getattr(sampler, "rho", 0.0)), float(sigma_data))
    hit = _PLAN_CACHE.get(key)
    if hit is not None:
        return sigmas, hit                               # (a tuple: every caller shares it)
    steps: List[StepScalars] = []
    for i in range(num_steps - 1):
        sigma, sigma_next = sigmas[i], sigmas[i + 1]
        sigma_up, sigma_down, sigma_mid = sampler.get_sigmas(sigma, sigma_next)
        dt_mid = sigma_mid - sigma                       # 0-dim fp32
        dt_down = sigma_down - sigma                     # python double - fp32 tensor -> fp32 tensor
        up32 = torch.tensor(sigma_up, dtype=torch.float32)
        renoise = math.sqrt(sigmas[i] ** 2 - sigmas[i + 1] ** 2)
        steps.append(StepScalars(float(sigma), float(sigma_mid), float(up32), float(dt_mid), float(dt_down),
                                 scale_weights(sigma, sigma_data), scale_weights(sigma_mid, sigma_data),
                                 float(torch.tensor(renoise, dtype=torch.float32))))
    if len(_PLAN_CACHE) >= 16:
        _PLAN_CACHE.pop(next(iter(_PLAN_CACHE)))
    _PLAN_CACHE[key] = tuple(steps)
    return sigmas, _PLAN_CACHE[key]


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


def _plan_sigmas(num_steps: int, schedule) -> Tensor:
    return schedule.detach().float().cpu() if isinstance(schedule, torch.Tensor) else schedule(num_steps)


def _plan_store(key, steps) -> tuple:
    if len(_PLAN_CACHE) >= 16:
        _PLAN_CACHE.pop(next(iter(_PLAN_CACHE)))
    _PLAN_CACHE[key] = tuple(steps)
    return _PLAN_CACHE[key]


def aeuler_plan(num_steps: int, schedule, sampler: AEulerSampler, sigma_data: float):
    """Per-step scalars of AEulerSampler.forward/step (diffusion.py:465-483), bit for bit as the reference computes them on
    CPU; ``schedule`` and the cache as adpm2_plan.  One time row per step."""
    sigmas = _plan_sigmas(num_steps, schedule)
    key = (num_steps, sigmas.numpy().tobytes(), type(sampler), (), float(sigma_data))
    hit = _PLAN_CACHE.get(key)
    if hit is not None:
        return sigmas, hit
    steps: List[AEulerStep] = []
    for i in range(num_steps - 1):
        sigma, sigma_next = sigmas[i], sigmas[i + 1]
        sigma_up, sigma_down = sampler.get_sigmas(sigma, sigma_next)
        dt = sigma_down - sigma                          # python double - fp32 tensor -> fp32 tensor
        up32 = torch.tensor(sigma_up, dtype=torch.float32)
        steps.append(AEulerStep(float(sigma), float(up32), float(dt), scale_weights(sigma, sigma_data)))
    return sigmas, _plan_store(key, steps)


def karras_plan(num_steps: int, schedule, sampler: KarrasSampler, sigma_data: float):
    """Per-step scalars of KarrasSampler.forward/step (diffusion.py:417-453), bit for bit as the reference computes them on
    CPU; ``schedule`` and the cache as adpm2_plan.  Two time rows per step, one when sigma_next == 0 (reachable with an
    evaluated sigma tensor that ends in 0; a KarrasSchedule's padded 0 is never reached)."""
    sigmas = _plan_sigmas(num_steps, schedule)
    params = (float(sampler.s_tmin), float(sampler.s_tmax), float(sampler.s_churn), float(sampler.s_noise))
    key = (num_steps, sigmas.numpy().tobytes(), type(sampler), params, float(sigma_data))
    hit = _PLAN_CACHE.get(key)
    if hit is not None:
        return sigmas, hit
    gammas = sampler.get_gammas(sigmas, num_steps)
    s_noise32 = float(torch.tensor(sampler.s_noise, dtype=torch.float32))     # python double * fp32 tensor: rounded first
    steps: List[KarrasStep] = []
    rows = 0
    for i in range(num_steps - 1):
        sigma, sigma_next, gamma = sigmas[i], sigmas[i + 1], gammas[i]
        sigma_hat = sigma + gamma * sigma                                     # 0-dim fp32
        ns32 = torch.tensor(math.sqrt(sigma_hat ** 2 - sigma ** 2), dtype=torch.float32)
        dt = sigma_next - sigma_hat
        half = 0.5 * (sigma - sigma_hat)
        euler_only = not bool(sigma_next != 0)
        steps.append(KarrasStep(float(sigma), float(sigma_next), float(gamma), float(sigma_hat), float(ns32), s_noise32,
                                float(dt), float(half), scale_weights(sigma_hat, sigma_data),
                                None if euler_only else scale_weights(sigma_next, sigma_data), euler_only,
                                rows, -1 if euler_only else rows + 1))
        rows += 1 if euler_only else 2
    return sigmas, _plan_store(key, steps)


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
    """

    def __init__(self, init: Optional[Tensor] = None, steps: Optional[Callable[[int], Tensor]] = None,
                 seed: Optional[int] = None, sample0: int = 0):
        if (init is None) != (steps is None) or (init is None) == (seed is None):
            raise ValueError("give either (init, steps) tensors or a seed")
        self.init, self.steps, self.seed, self.sample0 = init, steps, seed, sample0


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
    def forward(self, inpaint: Tensor, inpaint_mask: Tensor, *, draw=None, seed=None, **kwargs) -> Tensor:
        fn = BoundDenoise(self.denoise_fn, kwargs, dict(draw=draw, seed=seed))
        return self.inpaint_fn(source=inpaint, mask=inpaint_mask, fn=fn, sigmas=self.sigma_schedule(self.num_steps, inpaint.device),
                               num_steps=self.num_steps, num_resamples=self.num_resamples)


# ----------------------------------------------------------------------------------------------
# the fused sampling loop
# ----------------------------------------------------------------------------------------------
def _f32(t: Tensor, device) -> Tensor:
    return t.to(device=device, dtype=torch.float32).contiguous()


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


def _guided_eval(engine, lib, B: int, guided: bool, dual: bool, embedding_scale: float, st) -> Tensor:
    """net(x, t, embedding, embedding_scale) of engine.xin[:B] -> prediction rows [:B] (UNetCFG1d.forward)."""
    if dual:
        engine.xin[B:].copy_(engine.xin[:B], non_blocking=True)
        both = engine.eval(dual=True)
        pred, um = both[:B], both[B:]
    else:
        pred = engine.eval(False)
        um = engine.eval(True) if guided else None
    if guided:
        rt.check(lib.mdt_cfg_mix(rt.ptr(pred), rt.ptr(um), rt.ptr(pred), float(embedding_scale), pred.numel(), st))
    return pred


def run_adpm2(engine, embedding: Tensor, pred_dim: int, num_steps: int, noise: NoiseSource,
              schedule, sampler: ADPM2Sampler, sigma_data: float, embedding_scale: float = 1.0,
              clamp: bool = False, trace: Optional[dict] = None, timer=None, tokens: Optional[Tensor] = None,
              dynamic_threshold: float = 0.0) -> Tensor:
    """DiffusionSampler.forward (diffusion.py:577-591) + ADPM2Sampler.forward (:517-524) +
    KDiffusion_mod.denoise_fn (:798-814) + UNetCFG1d.forward (modules.py:1228-1255) on the GPU.
    ``tokens`` (B, L) int32: also the decode step after the path, argmax over channels of the final sample
    (generative.py:1212-1213), written by the last update kernel."""
    lib = rt.load_library()
    dev = engine.device
    B = embedding.shape[0]
    C, L, Cp = pred_dim, engine.c.length, engine.c.in_pad
    sigmas, steps = adpm2_plan(num_steps, schedule, sampler, sigma_data)
    guided = embedding_scale != 1.0

    with torch.cuda.device(dev):
        st = rt.current_stream()
        engine.handoff_check()                        # a time-out of the previous call's pair hand-offs is reported here
        dual = _guided_setup(engine, embedding, guided)
        c_noise = torch.tensor([v for s in steps for v in (s.w.c_noise, s.w_mid.c_noise)], dtype=torch.float32)
        engine.prepare_times(c_noise)

        x = torch.empty(B, C, L, device=dev)
        x_mid = torch.empty_like(x)
        seed = noise.seed or 0
        dscale = torch.empty(B, device=dev) if dynamic_threshold else None      # clip()'s per-sample dynamic threshold

        def dyn(xs, pred, w):
            if dscale is not None:
                rt.check(lib.mdt_dyn_scale(rt.ptr(xs), rt.ptr(pred), rt.ptr(dscale), w.c_skip, w.c_out, float(dynamic_threshold),
                                           B, C, L, Cp, st))
            return rt.ptr(dscale)
        init = None if noise.init is None else _f32(noise.init, dev)
        rt.check(lib.mdt_init_noise(rt.ptr(x), rt.ptr(init), float(sigmas[0]), seed, 0, noise.sample0, B, C, L, st))
        if not steps:
            x = x.clamp(-1.0, 1.0) if clamp else x
            if tokens is not None:
                rt.check(lib.mdt_argmax_tokens(rt.ptr(x), rt.ptr(tokens), B, C, L, st))
            return x
        rt.check(lib.mdt_precond_in(rt.ptr(x), rt.ptr(engine.xin), steps[0].w.c_in, B, C, L, Cp, st))

        def unet(row: int) -> Tensor:
            engine.select_time(row)
            if timer is not None:
                timer.start()
            pred = _guided_eval(engine, lib, B, guided, dual, embedding_scale, st)
            if timer is not None:
                timer.stop()
            return pred

        for i, s in enumerate(steps):
            pred = unet(2 * i)
            rt.check(lib.mdt_adpm2_mid(rt.ptr(x), rt.ptr(pred), rt.ptr(x_mid), rt.ptr(engine.xin), s.w.c_skip,
                                       s.w.c_out, s.sigma, s.dt_mid, s.w_mid.c_in, B, C, L, Cp, dyn(x, pred, s.w), st))
            pred = unet(2 * i + 1)
            nz = None if noise.steps is None else _f32(noise.steps(i), dev)
            last = i + 1 == len(steps)
            c_in_next = 0.0 if last else steps[i + 1].w.c_in
            rt.check(lib.mdt_adpm2_next(rt.ptr(x), rt.ptr(x_mid), rt.ptr(pred), rt.ptr(nz),
                                        0 if last else rt.ptr(engine.xin), s.w_mid.c_skip, s.w_mid.c_out,
                                        s.sigma_mid, s.dt_down, s.sigma_up, c_in_next, seed, i + 1, noise.sample0,
                                        B, C, L, Cp, rt.ptr(tokens) if (last and not clamp) else 0, dyn(x_mid, pred, s.w_mid), st))
            if trace is not None and (i + 1) in trace.get("want", ()):
                trace[i + 1] = x.clone()
        if clamp:
            rt.check(lib.mdt_clamp(rt.ptr(x), -1.0, 1.0, x.numel(), st))
            if tokens is not None:        # clamping creates ties (first maximum wins): decode the clamped sample
                rt.check(lib.mdt_argmax_tokens(rt.ptr(x), rt.ptr(tokens), B, C, L, st))
        engine.note_handoff()
    return x


class _Loop:
    """What run_aeuler / run_karras share with run_adpm2's prologue and epilogue: context and time table, the state
    initialised from the first draw, the timed guided evaluation, the per-sample dynamic threshold, final clamp and decode."""

    def __init__(self, engine, embedding, pred_dim, noise, sigmas, steps, embedding_scale, timer, dynamic_threshold):
        self.lib, self.engine, self.noise, self.timer = rt.load_library(), engine, noise, timer
        self.B, self.C, self.L, self.Cp = embedding.shape[0], pred_dim, engine.c.length, engine.c.in_pad
        self.scale, self.guided, self.q = embedding_scale, embedding_scale != 1.0, float(dynamic_threshold)
        self.st = rt.current_stream()
        engine.handoff_check()                        # a time-out of the previous call's pair hand-offs is reported here
        self.dual = _guided_setup(engine, embedding, self.guided)
        engine.prepare_times(torch.tensor(plan_time_rows(steps), dtype=torch.float32))
        self.x = torch.empty(self.B, self.C, self.L, device=engine.device)
        self.seed = noise.seed or 0
        self.dscale = torch.empty(self.B, device=engine.device) if dynamic_threshold else None
        init = None if noise.init is None else _f32(noise.init, engine.device)
        rt.check(self.lib.mdt_init_noise(rt.ptr(self.x), rt.ptr(init), float(sigmas[0]), self.seed, 0, noise.sample0,
                                         self.B, self.C, self.L, self.st))

    def dims(self):
        return self.B, self.C, self.L, self.Cp

    def draw(self, i: int) -> Optional[Tensor]:
        """The explicit torch.randn_like draw of step i, or None for the counter-based generator (draw index i + 1)."""
        return None if self.noise.steps is None else _f32(self.noise.steps(i), self.engine.device)

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

    def finish(self, x: Tensor, clamp: bool, tokens: Optional[Tensor], decoded: bool, handoff: bool = True) -> Tensor:
        """Final clamp (mdt_clamp) and the decode when the last update kernel has not done it."""
        if clamp:
            rt.check(self.lib.mdt_clamp(rt.ptr(x), -1.0, 1.0, x.numel(), self.st))
        if tokens is not None and (clamp or not decoded):   # clamping creates ties (first maximum wins): decode the clamped sample
            rt.check(self.lib.mdt_argmax_tokens(rt.ptr(x), rt.ptr(tokens), self.B, self.C, self.L, self.st))
        if handoff:
            self.engine.note_handoff()
        return x


def run_aeuler(engine, embedding: Tensor, pred_dim: int, num_steps: int, noise: NoiseSource,
               schedule, sampler: AEulerSampler, sigma_data: float, embedding_scale: float = 1.0,
               clamp: bool = False, trace: Optional[dict] = None, timer=None, tokens: Optional[Tensor] = None,
               dynamic_threshold: float = 0.0) -> Tensor:
    """DiffusionSampler.forward (diffusion.py:577-591) + AEulerSampler.forward (:476-483) + KDiffusion_mod.denoise_fn
    (:798-814) + UNetCFG1d.forward (modules.py:1228-1255) on the GPU: run_adpm2's arguments and structure, one evaluation
    and one mdt_aeuler_next launch per step."""
    sigmas, steps = aeuler_plan(num_steps, schedule, sampler, sigma_data)
    with torch.cuda.device(engine.device):
        lp = _Loop(engine, embedding, pred_dim, noise, sigmas, steps, embedding_scale, timer, dynamic_threshold)
        lib, x, st = lp.lib, lp.x, lp.st
        if not steps:
            return lp.finish(x, clamp, tokens, False, handoff=False)
        rt.check(lib.mdt_precond_in(rt.ptr(x), rt.ptr(engine.xin), steps[0].w.c_in, *lp.dims(), st))
        for i, s in enumerate(steps):
            pred = lp.unet(i)
            nz = lp.draw(i)
            last = i + 1 == len(steps)
            c_in_next = 0.0 if last else steps[i + 1].w.c_in
            rt.check(lib.mdt_aeuler_next(rt.ptr(x), rt.ptr(pred), rt.ptr(nz), 0 if last else rt.ptr(engine.xin), s.w.c_skip,
                                         s.w.c_out, s.sigma, s.dt, s.sigma_up, c_in_next, lp.seed, i + 1, noise.sample0,
                                         *lp.dims(), rt.ptr(tokens) if (last and not clamp) else 0, lp.dyn(x, pred, s.w), st))
            if trace is not None and (i + 1) in trace.get("want", ()):
                trace[i + 1] = x.clone()
        return lp.finish(x, clamp, tokens, True)


def run_karras(engine, embedding: Tensor, pred_dim: int, num_steps: int, noise: NoiseSource,
               schedule, sampler: KarrasSampler, sigma_data: float, embedding_scale: float = 1.0,
               clamp: bool = False, trace: Optional[dict] = None, timer=None, tokens: Optional[Tensor] = None,
               dynamic_threshold: float = 0.0) -> Tensor:
    """DiffusionSampler.forward (diffusion.py:577-591) + KarrasSampler.forward (:437-453) + KDiffusion_mod.denoise_fn
    (:798-814) + UNetCFG1d.forward (modules.py:1228-1255) on the GPU: run_adpm2's arguments.  Per step: mdt_karras_hat
    (churn; in place on x), evaluation at sigma_hat, mdt_karras_mid, evaluation at sigma_next, mdt_karras_next."""
    sigmas, steps = karras_plan(num_steps, schedule, sampler, sigma_data)
    with torch.cuda.device(engine.device):
        lp = _Loop(engine, embedding, pred_dim, noise, sigmas, steps, embedding_scale, timer, dynamic_threshold)
        lib, x, st = lp.lib, lp.x, lp.st
        if not steps:
            return lp.finish(x, clamp, tokens, False, handoff=False)
        d, x_next = torch.empty_like(x), torch.empty_like(x)
        for i, s in enumerate(steps):
            nz = lp.draw(i)
            rt.check(lib.mdt_karras_hat(rt.ptr(x), rt.ptr(nz), rt.ptr(x), rt.ptr(engine.xin), s.noise_scale, s.s_noise,
                                        s.w_hat.c_in, lp.seed, i + 1, noise.sample0, *lp.dims(), st))      # x is x_hat from here
            pred = lp.unet(s.row_hat)
            tok = rt.ptr(tokens) if (i + 1 == len(steps) and not clamp) else 0
            if s.euler_only:
                rt.check(lib.mdt_karras_mid(rt.ptr(x), rt.ptr(pred), rt.ptr(d), rt.ptr(x_next), 0, s.w_hat.c_skip, s.w_hat.c_out,
                                            s.sigma_hat, s.dt, 0.0, *lp.dims(), tok, lp.dyn(x, pred, s.w_hat), st))
                x, x_next = x_next, x
            else:
                rt.check(lib.mdt_karras_mid(rt.ptr(x), rt.ptr(pred), rt.ptr(d), rt.ptr(x_next), rt.ptr(engine.xin), s.w_hat.c_skip,
                                            s.w_hat.c_out, s.sigma_hat, s.dt, s.w_next.c_in, *lp.dims(), 0,
                                            lp.dyn(x, pred, s.w_hat), st))
                pred = lp.unet(s.row_next)
                rt.check(lib.mdt_karras_next(rt.ptr(x), rt.ptr(x_next), rt.ptr(d), rt.ptr(pred), rt.ptr(x), s.w_next.c_skip,
                                             s.w_next.c_out, s.sigma_next, s.half, *lp.dims(), tok,
                                             lp.dyn(x_next, pred, s.w_next), st))
            if trace is not None and (i + 1) in trace.get("want", ()):
                trace[i + 1] = x.clone()
        return lp.finish(x, clamp, tokens, True)


def run_adpm2_inpaint(engine, embedding: Tensor, source: Tensor, mask: Tensor, num_steps: int, num_resamples: int,
                      draw: Optional[Callable[[], Tensor]], seed: Optional[int], schedule,
                      sampler: ADPM2Sampler, sigma_data: float, embedding_scale: float = 1.0,
                      sample0: int = 0, dynamic_threshold: float = 0.0) -> Tensor:
    """ADPM2Sampler.inpaint (diffusion.py:526-549) behind DiffusionInpainter.forward (:612-625).
    ``draw()`` returns the next torch.randn_like tensor in the reference's call order (parity mode);
    otherwise draws come from the counter-based generator keyed by (seed, draw index)."""
    lib = rt.load_library()
    dev = engine.device
    B, C, L = source.shape
    Cp = engine.c.in_pad
    sigmas, steps = adpm2_plan(num_steps, schedule, sampler, sigma_data)
    guided = embedding_scale != 1.0
    if mask.dtype != torch.bool or tuple(mask.shape) != tuple(source.shape):
        raise ValueError("in_paint_mask must be a bool tensor of the same shape as inpaint")

    counter = {"n": 0}

    def next_draw():
        counter["n"] += 1
        return (None if draw is None else _f32(draw(), dev)), counter["n"] - 1

    with torch.cuda.device(dev):
        st = rt.current_stream()
        engine.handoff_check()
        dual = _guided_setup(engine, embedding, guided)
        c_noise = torch.tensor([v for s in steps for v in (s.w.c_noise, s.w_mid.c_noise)], dtype=torch.float32)
        engine.prepare_times(c_noise)
        src = _f32(source, dev)
        mk = mask.to(device=dev).to(torch.uint8).contiguous()
        x = torch.empty(B, C, L, device=dev)
        x_mid = torch.empty_like(x)
        dscale = torch.empty(B, device=dev) if dynamic_threshold else None

        def dyn(xs, pred, w):
            if dscale is not None:
                rt.check(lib.mdt_dyn_scale(rt.ptr(xs), rt.ptr(pred), rt.ptr(dscale), w.c_skip, w.c_out, float(dynamic_threshold),
                                           B, C, L, Cp, st))
            return rt.ptr(dscale)
        sd = seed or 0
        nz, k = next_draw()
        rt.check(lib.mdt_init_noise(rt.ptr(x), rt.ptr(nz), float(sigmas[0]), sd, k, sample0, B, C, L, st))

        def unet(row: int) -> Tensor:
            engine.select_time(row)
            return _guided_eval(engine, lib, B, guided, dual, embedding_scale, st)

        for i, s in enumerate(steps):
            src_nz, src_k = next_draw()                   # source_noisy = source + sigmas[i] * randn_like(source)
            for r in range(num_resamples):
                rt.check(lib.mdt_inpaint_merge(rt.ptr(x), rt.ptr(src), rt.ptr(mk), rt.ptr(src_nz), s.sigma, sd,
                                               src_k, sample0, B, C, L, st))
                rt.check(lib.mdt_precond_in(rt.ptr(x), rt.ptr(engine.xin), s.w.c_in, B, C, L, Cp, st))
                pred = unet(2 * i)
                rt.check(lib.mdt_adpm2_mid(rt.ptr(x), rt.ptr(pred), rt.ptr(x_mid), rt.ptr(engine.xin), s.w.c_skip,
                                           s.w.c_out, s.sigma, s.dt_mid, s.w_mid.c_in, B, C, L, Cp, dyn(x, pred, s.w), st))
                pred = unet(2 * i + 1)
                nz, k = next_draw()
                rt.check(lib.mdt_adpm2_next(rt.ptr(x), rt.ptr(x_mid), rt.ptr(pred), rt.ptr(nz), 0, s.w_mid.c_skip,
                                            s.w_mid.c_out, s.sigma_mid, s.dt_down, s.sigma_up, 0.0, sd, k, sample0,
                                            B, C, L, Cp, 0, dyn(x_mid, pred, s.w_mid), st))
                if r < num_resamples - 1:
                    nz, k = next_draw()
                    rt.check(lib.mdt_add_noise(rt.ptr(x), rt.ptr(nz), s.renoise, sd, k, sample0, B, C, L, st))
        rt.check(lib.mdt_inpaint_merge(rt.ptr(x), rt.ptr(src), rt.ptr(mk), 0, 0.0, sd, 0, sample0, B, C, L, st))
        engine.note_handoff()
    return x
