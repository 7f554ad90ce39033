#!/usr/bin/env python3
"""A guidance sweep as ONE fused call (guidance_sweep: a guidance scale per sample, batch S * B) beside the S scalar sample()
calls of batch B it replaces -- the reference's `for s in cond_scales: model.sample(..., cond_scale=s)` -- on the configs[1]
model (64 timesteps, ADPM2, inputs resident, on-device counter-based noise):

    python tools/bench_guidance_sweep.py [--timesteps 64] [--steps 3] [--warmup 1] [--scales 1,1.5,...]      -> one JSON line

Two sweeps, each of 8 scales: over 128 conditionings and over 16.  Both forms of a sweep are measured in the same child process
(one per sweep, under --leg-timeout seconds; the first failing leg ends the run: no further process is started on the GPU
after a fault, an abort or a time-out), in ms per sweep and molecules/s.  The default scales hold 1.0, as the reference's sweeps
do: its scalar call runs unguided (half the evaluations, and an engine batch of its own, so the evaluation graphs are captured
anew on the way in and out), while the one-call form pays the unconditional pass for those rows too; --scales without 1.0
leaves both effects out.

    python tools/bench_guidance_sweep.py --leg 8x16

measures one sweep in the calling process (e.g. under a kernel trace).
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

SCALES = (1.0, 1.5, 2.0, 3.0, 4.0, 5.0, 7.5, 10.0)
LEGS = {"8x128": 128, "8x16": 16}          # sweep -> conditionings


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--timesteps", type=int, default=64)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--scales", type=lambda v: tuple(float(x) for x in v.split(",")), default=SCALES,
                    help="the guidance scales of a sweep, comma-separated (default: %(default)s)")
    ap.add_argument("--leg", choices=tuple(LEGS), default=None, help="measure this sweep in the calling process")
    ap.add_argument("--leg-timeout", type=int, default=240)
    return ap.parse_args()


def run_leg(a):
    import torch
    from moleculediffusiontransformer_amd import NoiseSource, guidance_sweep
    from moleculediffusiontransformer_amd.synth import make_synth_model, synth_normal
    if not torch.cuda.is_available():
        raise SystemExit("bench_guidance_sweep.py needs an MI355X: the sampling path has no CPU fallback")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    with contextlib.redirect_stdout(sys.stderr):
        model = make_synth_model("cfg1", device)
    B, T, S = LEGS[a.leg], a.timesteps, len(a.scales)
    seq = synth_normal("bench/seq/rank0", (B, model.unet.config.ctx_max_length)).to(device)

    def one_call(i):
        return guidance_sweep(model, seq, a.scales, device, timesteps=T, noise=NoiseSource(seed=1234 + i))

    def scalar_calls(i):
        return torch.stack([model.sample(seq, device, cond_scale=s, timesteps=T, noise=NoiseSource(seed=1234 + i, sample0=k * B))
                            for k, s in enumerate(a.scales)])

    def measure(form):
        for w in range(a.warmup):
            form(w)
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        for k in range(a.steps):
            out = form(a.warmup + k)
        torch.cuda.synchronize(device)
        dt = (time.perf_counter() - t0) / a.steps
        assert out.shape[:2] == (S, B) and bool(torch.isfinite(out).all())
        return {"ms_per_sweep": 1e3 * dt, "molecules_per_s": S * B / dt}, out
    scalar, want = measure(scalar_calls)
    fused, got = measure(one_call)
    again, _ = measure(scalar_calls)                 # the scalar form once more, after the one-call form: drift of the box
    return {"scales": list(a.scales), "conditionings": B, "rows_per_sweep": S * B, "one_call": fused, "scalar_calls": scalar,
            "scalar_calls_again": again, "one_call_speedup": scalar["ms_per_sweep"] / fused["ms_per_sweep"],
            "max_abs_difference": float((got - want).abs().max())}


def main():
    a = parse()
    if a.leg:
        print(json.dumps(run_leg(a)), flush=True)
        return 0
    result = {"metric": "guidance sweep at configs[1]: one fused call against S scalar calls", "timesteps": a.timesteps,
              "steps": a.steps, "warmup": a.warmup, "legs": {}}
    for leg in LEGS:
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--timesteps", str(a.timesteps), "--steps", str(a.steps),
               "--warmup", str(a.warmup), "--scales", ",".join(str(v) for v in a.scales)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.leg_timeout)
        except subprocess.TimeoutExpired:
            result["failed"] = f"{leg}: no result within {a.leg_timeout} s"
            break
        if r.returncode != 0:
            result["failed"] = f"{leg}: exit status {r.returncode}: {r.stderr.strip().splitlines()[-1:]}"
            break
        result["legs"][leg] = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(result), flush=True)
    return 1 if "failed" in result else 0


if __name__ == "__main__":
    sys.exit(main())
