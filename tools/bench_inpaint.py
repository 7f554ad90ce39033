#!/usr/bin/env python3
"""ms per call and molecules/s of draft completion at BASELINE configs[1] (B = 1024, 64 timesteps, inputs resident, on-device
counter-based noise, cond_scale 1.0), num_resamples 1 and 2: the dense inpaint() on the one-hot draft and the full-shape mask, and
inpaint_tokens() on the draft ids and the per-position mask.

    python tools/bench_inpaint.py [--batch 1024] [--timesteps 64] [--steps 3] [--warmup 1] [--forms dense,tokens]   -> one JSON line

Every leg (form x num_resamples) is measured in a child process of its own under a time limit (--leg-timeout seconds); the first
failing leg ends the run (no further process is started on the GPU after a fault, an abort or a time-out).  `--forms dense` runs on
a tree that has no inpaint_tokens() yet (an A/B against an older commit).  `--leg dense:2` measures one leg in the calling process.

"update_launches_per_resample": the launches of the loop's own kernels (merge / re-noise / input scaling / mdt_inpaint_enter, the
two ADPM2 update kernels, and the one closing merge of a call) one call makes, counted at the C ABI, over its
(timesteps - 1) * num_resamples resamples; the U-Net evaluations (two per resample) are not counted.
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

FORMS = ("dense", "tokens")
RESAMPLES = (1, 2)
LOOP_KERNELS = ("mdt_inpaint_enter", "mdt_inpaint_finish", "mdt_inpaint_merge", "mdt_add_noise", "mdt_precond_in", "mdt_adpm2_mid",
                "mdt_adpm2_next")
KEPT = 0.5            # fraction of positions kept


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--timesteps", type=int, default=64)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--forms", default=",".join(FORMS), help="comma-separated: dense, tokens")
    ap.add_argument("--leg", default=None, help="FORM:NUM_RESAMPLES: measure this leg in the calling process")
    ap.add_argument("--leg-timeout", type=int, default=240)
    return ap.parse_args()


def run_leg(a):
    import torch
    from moleculediffusiontransformer_amd import runtime as rt
    from moleculediffusiontransformer_amd.synth import make_synth_model, synth_normal
    form, R = a.leg.split(":")[0], int(a.leg.split(":")[1])
    if not torch.cuda.is_available():
        raise SystemExit("bench_inpaint.py needs an MI355X: the sampling path has no CPU fallback")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    with contextlib.redirect_stdout(sys.stderr):
        model = make_synth_model("cfg1", device)
    B, T, C, L = a.batch, a.timesteps, model.pred_dim, model.max_length
    seq = synth_normal("bench/seq/rank0", (B, model.unet.config.ctx_max_length)).to(device)
    draft = torch.randint(0, C, (B, L), generator=torch.Generator().manual_seed(7)).to(device)
    keep = (torch.rand(B, L, generator=torch.Generator().manual_seed(8)) < KEPT).to(device)
    if form == "dense":             # what a caller of inpaint() builds (generative.py:1567-1569, :1600-1603); resident, not timed
        src = torch.where(draft.unsqueeze(1) == torch.arange(C, device=device).view(1, C, 1), 1.0, -1.0).float().contiguous()
        mask = keep.unsqueeze(1).expand(-1, C, -1).contiguous()

        def step(i):
            return model.inpaint(seq, device, cond_scale=1.0, timesteps=T, num_resamples=R, inpaint=src, in_paint_mask=mask,
                                 seed=1234 + i)
    else:
        def step(i):
            return model.inpaint_tokens(seq, device, draft, keep, cond_scale=1.0, timesteps=T, num_resamples=R, seed=1234 + i)
    for w in range(a.warmup):
        step(w)
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    for k in range(a.steps):
        out = step(a.warmup + k)
    torch.cuda.synchronize(device)
    dt = time.perf_counter() - t0
    assert out.shape[0] == B and (out.is_floating_point() is (form == "dense"))
    if form == "dense":
        assert torch.isfinite(out).all()
    # one more call, untimed, with the loop's own C ABI entries counted
    lib, counts = rt.load_library(), {}
    for name in LOOP_KERNELS:
        fn = getattr(lib, name, None)
        if fn is not None:
            def counted(*args, _fn=fn, _name=name):
                counts[_name] = counts.get(_name, 0) + 1
                return _fn(*args)
            setattr(lib, name, counted)
    step(a.warmup + a.steps)
    torch.cuda.synchronize(device)
    resamples = max((T - 1) * R, 1)
    return {"form": form, "num_resamples": R, "ms_per_call": 1e3 * dt / a.steps, "molecules_per_s": B * a.steps / dt,
            "ms_per_resample": 1e3 * dt / a.steps / resamples, "update_launches_per_resample": sum(counts.values()) / resamples,
            "update_launches_per_call": counts}


def main():
    a = parse()
    if a.leg:
        print(json.dumps(run_leg(a)), flush=True)
        return 0
    forms = [f for f in a.forms.split(",") if f]
    if not forms or any(f not in FORMS for f in forms):
        raise SystemExit(f"--forms takes a comma-separated subset of {FORMS}")
    result = {"metric": "draft completion at configs[1]", "batch": a.batch, "timesteps": a.timesteps, "steps": a.steps,
              "warmup": a.warmup, "kept_fraction": KEPT, "legs": {}}
    for leg in [f"{f}:{r}" for f in forms for r in RESAMPLES]:
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
