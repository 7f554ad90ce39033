#!/usr/bin/env python3
"""ms per sample() call and molecules/s of the three fused sampler loops at BASELINE configs[1] (B = 1024, 64 timesteps,
inputs resident, on-device counter-based noise, cond_scale 1.0) -- bench.py's headline workload and step definition, with
the sampler chosen:

    python tools/bench_samplers.py [--batch 1024] [--timesteps 64] [--steps 3] [--warmup 1]      -> one JSON line

Every sampler is measured in a child process of its own under a time limit (--leg-timeout seconds); the first failing leg
ends the run (no further process is started on the GPU after a fault, an abort or a time-out).  The ADPM2 leg is the same
call bench.py times and should agree with its line on the same box.

    rocprofv3 --output-format csv --kernel-trace --stats -d DIR -o run -- python tools/bench_samplers.py --leg aeuler

times one leg in the calling process, for a kernel trace of its own (k_aeuler_next / k_karras_* in kernel_stats.csv).
`--update-batch N` (default 8192, bench.py's size for this class; 0 = off) adds the update kernels alone, HIP-event timed over
50 launches each by bench.py's method (algorithmic bytes = every tensor read or written once), k_adpm2_next beside them.
"""
import argparse
import contextlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KARRAS = (0.05, 5.0, 4.0, 1.003)           # s_tmin, s_tmax, s_churn, s_noise of the Karras leg
LEGS = ("adpm2", "aeuler", "karras")
HBM_PEAK_GBS = 8000.0


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--timesteps", type=int, default=64)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--leg", choices=LEGS + ("updates",), default=None, help="measure this leg in the calling process")
    ap.add_argument("--update-batch", type=int, default=8192)
    ap.add_argument("--leg-timeout", type=int, default=240)
    return ap.parse_args()


def run_leg(a):
    import torch
    from moleculediffusiontransformer_amd import ADPM2Sampler, AEulerSampler, KarrasSampler, NoiseSource
    from moleculediffusiontransformer_amd.synth import make_synth_model, synth_normal
    if not torch.cuda.is_available():
        raise SystemExit("bench_samplers.py needs an MI355X: the sampling path has no CPU fallback")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    with contextlib.redirect_stdout(sys.stderr):
        model = make_synth_model("cfg1", device)
    B, T = a.batch, a.timesteps
    seq = synth_normal("bench/seq/rank0", (B, model.unet.config.ctx_max_length)).to(device)
    sampler = {"adpm2": lambda: ADPM2Sampler(rho=1), "aeuler": AEulerSampler, "karras": lambda: KarrasSampler(*KARRAS)}[a.leg]()
    evals = (T - 1) * (1 if a.leg == "aeuler" else 2)

    def step(i):
        return model.sample(seq, device, cond_scale=1.0, timesteps=T, clamp=False, noise=NoiseSource(seed=1234 + i),
                            sampler=sampler)
    for w in range(a.warmup):
        step(w)
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    for k in range(a.steps):
        out = step(a.warmup + k)
    torch.cuda.synchronize(device)
    dt = time.perf_counter() - t0
    assert torch.isfinite(out).all()
    return {"sampler": type(sampler).__name__, "unet_evaluations_per_call": evals, "ms_per_call": 1e3 * dt / a.steps,
            "molecules_per_s": B * a.steps / dt, "ms_per_timestep": 1e3 * dt / a.steps / (T - 1)}


def run_updates(a):
    """The update kernels alone at --update-batch samples of configs[1]'s shape, counter-based noise as the loops use it."""
    import torch
    from moleculediffusiontransformer_amd import runtime as rt
    lib = rt.load_library()
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    B, C, L, Cp = a.update_batch, 16, 64, 16
    x, xm, d = (torch.randn(B, C, L, device=device) for _ in range(3))
    xn, nz = torch.empty_like(x), torch.randn(B, C, L, device=device)
    pred, xin = torch.randn(B, L, Cp, device=device), torch.empty(B, L, Cp, device=device)
    keep = (torch.rand(B, C, L, device=device) < 0.5).to(torch.uint8)        # k_inpaint_enter: a dense mask, half of it kept
    rows = torch.full((B,), 0.5, device=device)                              # k_noise_in_rows: sigma[b] and c_in[b]
    st = rt.current_stream()
    p = rt.ptr
    calls = (
        ("k_adpm2_next", 5, lambda: lib.mdt_adpm2_next(p(x), p(xm), p(pred), 0, p(xin), 0.5, 0.5, 1.0, -0.1, 0.01, 0.7, 9, 1, 0,
                                                       B, C, L, Cp, 0, 0, st)),
        ("k_aeuler_next", 4, lambda: lib.mdt_aeuler_next(p(x), p(pred), 0, p(xin), 0.5, 0.5, 1.0, -0.1, 0.01, 0.7, 9, 1, 0,
                                                         B, C, L, Cp, 0, 0, st)),
        # the same two with an explicit noise tensor (one more stream, no generator): separates HBM from Philox + Box-Muller
        ("k_adpm2_next, explicit noise", 6, lambda: lib.mdt_adpm2_next(p(x), p(xm), p(pred), p(nz), p(xin), 0.5, 0.5, 1.0, -0.1, 0.01,
                                                                       0.7, 0, 0, 0, B, C, L, Cp, 0, 0, st)),
        ("k_aeuler_next, explicit noise", 5, lambda: lib.mdt_aeuler_next(p(x), p(pred), p(nz), p(xin), 0.5, 0.5, 1.0, -0.1, 0.01, 0.7,
                                                                         0, 0, 0, B, C, L, Cp, 0, 0, st)),
        ("k_karras_hat", 3, lambda: lib.mdt_karras_hat(p(x), 0, p(x), p(xin), 0.01, 1.003, 0.7, 9, 1, 0, B, C, L, Cp, st)),
        ("k_karras_mid", 5, lambda: lib.mdt_karras_mid(p(x), p(pred), p(d), p(xn), p(xin), 0.5, 0.5, 1.0, -0.1, 0.7,
                                                       B, C, L, Cp, 0, 0, st)),
        ("k_karras_next", 5, lambda: lib.mdt_karras_next(p(x), p(xn), p(d), p(pred), p(x), 0.5, 0.5, 1.0, -0.01,
                                                         B, C, L, Cp, 0, 0, st)),
        # the tile kernels around the samplers: preconditioning, the first ADPM2 half, the inpaint and training entries
        ("k_adpm2_mid", 4, lambda: lib.mdt_adpm2_mid(p(x), p(pred), p(xm), p(xin), 0.5, 0.5, 1.0, -0.1, 0.7, B, C, L, Cp, 0, st)),
        ("k_precond_in", 2, lambda: lib.mdt_precond_in(p(x), p(xin), 0.7, B, C, L, Cp, st)),
        ("k_precond_out", 3, lambda: lib.mdt_precond_out(p(x), p(pred), p(xn), 0.5, 0.5, B, C, L, Cp, 0, st)),
        ("k_inpaint_enter", 4.25, lambda: lib.mdt_inpaint_enter(p(x), p(xin), p(d), 0, p(keep), 0, 0, 0, 0.01, 0.0, 0.7, 9, 1, 2, 0,
                                                                B, C, L, Cp, st)),
        ("k_noise_in_rows", 3, lambda: lib.mdt_noise_in_rows(p(d), 0, p(rows), p(rows), p(xn), p(xin), 9, 1, 0, B, C, L, Cp, st)))
    res = {"batch": B}
    for name, nbuf, call in calls:
        for _ in range(5):
            rt.check(call())
        tm = rt.EventTimer(1)
        tm.start()
        for _ in range(50):
            rt.check(call())
        tm.stop()
        us = tm.collect()[0] * 1e3 / 50
        nbytes = nbuf * B * C * L * 4
        res[name] = {"us_per_launch": round(us, 2), "algorithmic_mb": round(nbytes / 1e6, 1),
                     "gb_per_s": round(nbytes / (us * 1e-6) / 1e9, 0),
                     "hbm_peak_frac": round(nbytes / (us * 1e-6) / 1e9 / HBM_PEAK_GBS, 3)}
    torch.cuda.synchronize(device)
    return res


def main():
    a = parse()
    if a.leg:
        print(json.dumps(run_updates(a) if a.leg == "updates" else run_leg(a)), flush=True)
        return 0
    result = {"metric": "sampler loops at configs[1]", "batch": a.batch, "timesteps": a.timesteps, "steps": a.steps,
              "warmup": a.warmup, "karras_params": list(KARRAS), "legs": {}}
    for leg in LEGS + (("updates",) if a.update_batch > 0 else ()):
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--batch", str(a.batch), "--timesteps", str(a.timesteps),
               "--steps", str(a.steps), "--warmup", str(a.warmup), "--update-batch", str(a.update_batch)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.leg_timeout)
        except subprocess.TimeoutExpired:
            result["failed"] = f"{leg}: no result within {a.leg_timeout} s"
            break
        if r.returncode != 0:
            result["failed"] = f"{leg}: exit status {r.returncode}: {r.stderr.strip().splitlines()[-1:]}"
            break
        result["legs"][leg] = json.loads(r.stdout.strip().splitlines()[-1])
    legs = dict(result["legs"])
    if "updates" in legs:
        result["update_kernels"] = result["legs"].pop("updates")
        del legs["updates"]
    if "adpm2" in legs:
        for leg in legs:
            legs[leg]["time_vs_adpm2"] = legs[leg]["ms_per_call"] / legs["adpm2"]["ms_per_call"]
    print(json.dumps(result), flush=True)
    return 1 if "failed" in result else 0


if __name__ == "__main__":
    sys.exit(main())
