#!/usr/bin/env python3
"""ms per call of lead refinement at BASELINE configs[1] (B = 1024, 64 timesteps, inputs resident, on-device counter-based noise,
cond_scale 1.0): refine_tokens() at strength 0.25, 0.5 and 1.0 beside sample_tokens() of the same tree, and a sweep of 4 strengths
over 128 and over 16 leads as ONE strength_sweep() call beside its 4 scalar refine_tokens() calls; and the masked leg ("keep"):
refine_keep_tokens(keep_mask=) at the same three strengths beside the unmasked call at the same strength, and at start_step = 0 beside
inpaint_tokens() (num_resamples 1) on the same draft and mask -- every pair in one process, alternating.

    python tools/bench_refine.py [--batch 1024] [--timesteps 64] [--steps 3] [--warmup 1] [--legs calls,sweep:128,sweep:16,keep]   -> one JSON line

Every leg is measured in a child process of its own under a time limit (--leg-timeout seconds); the first failing leg ends the run
(no further process is started on the GPU after a fault, an abort or a time-out).  `--leg sweep:16` measures one leg in the calling
process.

What to expect (arguments, not thresholds): a scalar call runs T - 1 - k of the T - 1 steps, so it should cost close to that share of
a full call plus the one entry launch ("share_of_sample" beside "steps_share"); a per-sample call runs EVERY row from min(start), so
the sweep evaluates rows that have not started yet and can only win while its scalar calls underfill the GPU; a masked call adds
one elementwise launch per step (mdt_refine_keep_enter) and one at the end (mdt_inpaint_finish) to the unmasked call, and at start 0
runs inpaint_tokens()'s evaluations with mdt_refine_keep_enter in place of mdt_inpaint_enter.
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

LEGS = ("calls", "sweep:128", "sweep:16", "keep")
STRENGTHS = (0.25, 0.5, 1.0)
SWEEP = (0.25, 0.5, 0.75, 1.0)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--timesteps", type=int, default=64)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--legs", default=",".join(LEGS), help="comma-separated: calls, sweep:LEADS, keep")
    ap.add_argument("--leg", default=None, help="measure this leg in the calling process")
    ap.add_argument("--leg-timeout", type=int, default=300)
    return ap.parse_args()


def timed(torch, device, step, warmup, steps):
    for w in range(warmup):
        step(w)
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    for k in range(steps):
        out = step(warmup + k)
    torch.cuda.synchronize(device)
    return 1e3 * (time.perf_counter() - t0) / steps, out


def run_leg(a):
    import torch
    from moleculediffusiontransformer_amd import NoiseSource, refine_start, strength_sweep
    from moleculediffusiontransformer_amd.synth import make_synth_model, synth_normal
    if not torch.cuda.is_available():
        raise SystemExit("bench_refine.py needs an MI355X: the sampling path has no CPU fallback")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    with contextlib.redirect_stdout(sys.stderr):
        model = make_synth_model("cfg1", device)
    T, C, L = a.timesteps, model.pred_dim, model.max_length
    kind, _, leads = a.leg.partition(":")
    B = a.batch if kind in ("calls", "keep") else int(leads)
    seq = synth_normal("bench/seq/rank0", (B, model.unet.config.ctx_max_length)).to(device)
    draft = torch.randint(0, C, (B, L), generator=torch.Generator().manual_seed(7)).to(device)
    if kind == "calls":
        ms, tok = timed(torch, device, lambda i: model.sample_tokens(seq, device, cond_scale=1.0, timesteps=T,
                                                                     noise=NoiseSource(seed=1234 + i)), a.warmup, a.steps)
        assert tok.shape == (B, L)
        out = {"leg": a.leg, "batch": B, "sample_tokens_ms": ms, "refine_tokens": {}}
        for s in STRENGTHS:
            k = refine_start(T, s)
            ms_s, tok = timed(torch, device, lambda i: model.refine_tokens(seq, device, draft, strength=s, cond_scale=1.0, timesteps=T,
                                                                           noise=NoiseSource(seed=1234 + i)), a.warmup, a.steps)
            assert tok.shape == (B, L)
            out["refine_tokens"][str(s)] = {"start_step": k, "ms_per_call": ms_s, "share_of_sample": ms_s / ms,
                                            "steps_share": (T - 1 - k) / (T - 1)}
        return out
    if kind == "keep":
        keep = ((torch.arange(L) // 6) % 2 == 0).repeat(B, 1).to(device)        # half of the positions, changing inside groups of four
        out = {"leg": a.leg, "batch": B, "kept_share": float(keep.float().mean()), "refine_tokens": {}}

        def pair(plain, masked):
            """(ms plain, ms masked), each the smaller of two alternating rounds"""
            ms = [[], []]
            for _ in range(2):
                for j, step in enumerate((plain, masked)):
                    t, tok = timed(torch, device, step, a.warmup, a.steps)
                    assert tok.shape == (B, L)
                    ms[j].append(t)
            return min(ms[0]), min(ms[1])
        for s in STRENGTHS:
            more = dict(strength=s, cond_scale=1.0, timesteps=T)
            ms_plain, ms_keep = pair(lambda i: model.refine_tokens(seq, device, draft, noise=NoiseSource(seed=1234 + i), **more),
                                     lambda i: model.refine_keep_tokens(seq, device, draft, noise=NoiseSource(seed=1234 + i),
                                                                        keep_mask=keep, **more))
            out["refine_tokens"][str(s)] = {"start_step": refine_start(T, s), "ms_per_call": ms_plain, "keep_mask_ms_per_call": ms_keep,
                                            "keep_over_plain": ms_keep / ms_plain}
        ms_inp, ms_keep = pair(lambda i: model.inpaint_tokens(seq, device, draft, keep, cond_scale=1.0, timesteps=T, num_resamples=1,
                                                              seed=1234 + i),
                               lambda i: model.refine_keep_tokens(seq, device, draft, 0, cond_scale=1.0, timesteps=T,
                                                                  noise=NoiseSource(seed=1234 + i), keep_mask=keep))
        out["start_0"] = {"inpaint_tokens_ms": ms_inp, "refine_tokens_keep_mask_ms": ms_keep, "keep_over_inpaint": ms_keep / ms_inp}
        return out
    S = len(SWEEP)
    ms_sweep, tok = timed(torch, device, lambda i: strength_sweep(model, seq, draft, SWEEP, device, cond_scale=1.0, timesteps=T,
                                                                  noise=NoiseSource(seed=1234 + i)), a.warmup, a.steps)
    assert tok.shape == (S, B, L)

    def scalar_calls(i):
        return [model.refine_tokens(seq, device, draft, strength=s, cond_scale=1.0, timesteps=T,
                                    noise=NoiseSource(seed=1234 + i, sample0=n * B)) for n, s in enumerate(SWEEP)]
    ms_scalar, toks = timed(torch, device, scalar_calls, a.warmup, a.steps)
    assert len(toks) == S and toks[0].shape == (B, L)
    return {"leg": a.leg, "leads": B, "strengths": list(SWEEP), "sweep_ms": ms_sweep, "scalar_calls_ms": ms_scalar,
            "sweep_over_scalar": ms_sweep / ms_scalar}


def main():
    a = parse()
    if a.leg:
        print(json.dumps(run_leg(a)), flush=True)
        return 0
    legs = [x for x in a.legs.split(",") if x]
    if not legs or any(x not in ("calls", "keep") and not (x.startswith("sweep:") and x[6:].isdigit() and int(x[6:]) > 0) for x in legs):
        raise SystemExit("--legs takes a comma-separated list of: calls, sweep:LEADS, keep")
    result = {"metric": "lead refinement at configs[1]", "batch": a.batch, "timesteps": a.timesteps, "steps": a.steps,
              "warmup": a.warmup, "legs": {}}
    for leg in legs:
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--batch", str(a.batch), "--timesteps", str(a.timesteps),
               "--steps", str(a.steps), "--warmup", str(a.warmup)]
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
