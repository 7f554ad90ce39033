#!/usr/bin/env python3
"""The per-row evaluation form (one noise level per sample) at BASELINE configs[1]'s model, beside the shared-row program of the
same process:

    python tools/bench_eval_loss.py [--batch 1024] [--sigmas 64] [--kernel-batch 8192] [--repeats 20]      -> one JSON line

  * `eval` (shared FiLM row, the sampling program) and `eval_rows` (one row per sample) as HIP-graph replays: median ms, launches;
    the ops of `eval_rows` timed one by one (HIP events around each launch, no graph) and summed by kind -- the time of the
    ResNet launches is what chaining them inside k_res256 / k_tf128 could still save;
  * denoise_fn(sigmas = --sigmas distinct values) with batched=True against batched=False (one evaluation per value);
  * eval_loss() end to end at --batch;
  * the noising and the fused loss kernel at --kernel-batch samples beside mdt_adpm2_mid (existing code of the same traffic
    class), algorithmic bytes = every tensor read or written once, 50 launches between two events.

Medians over --repeats after 3 warm-up runs; every ratio is between numbers of this one process.
"""
import argparse
import contextlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0


def median_ms(fn, repeats, sync, warmup=3):
    for _ in range(warmup):
        fn()
    sync()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        sync()
        out.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--sigmas", type=int, default=64)
    ap.add_argument("--kernel-batch", type=int, default=8192)
    ap.add_argument("--repeats", type=int, default=20)
    a = ap.parse_args()
    import torch
    from moleculediffusiontransformer_amd import runtime as rt
    from moleculediffusiontransformer_amd.diffusion import scale_weights_rows
    from moleculediffusiontransformer_amd.synth import make_synth_model, synth_normal
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval_loss.py needs an MI355X: the kernels have no CPU fallback")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    lib = rt.load_library()
    with contextlib.redirect_stdout(sys.stderr):
        model = make_synth_model("cfg1", device)

    def sync():
        torch.cuda.synchronize(device)
    B = a.batch
    C, L = model.pred_dim, model.max_length
    n_ctx = model.unet.config.ctx_max_length
    seq = synth_normal("bench/seq/rank0", (B, n_ctx))
    gen = torch.Generator().manual_seed(7)
    sig = (-1.2 + 1.2 * torch.randn(B, generator=gen)).exp()
    x0 = (0.5 * torch.randn(B, C, L, generator=gen)).clamp(-1, 1)
    emb = model._embed(seq, device)
    w = scale_weights_rows(sig, 0.1)
    res = {"metric": "per-row evaluation at configs[1]", "batch": B, "gemm_mode": model.gemm_mode, "repeats": a.repeats}

    # ---- eval (shared row) beside eval_rows, same batch, same inputs ----
    shared, rows = model.engine(device, n_ctx, B), model.engine(device, n_ctx, B, rows=True)
    for eng in (shared, rows):
        eng.reserve(B)
        eng.prepare_context(emb)
        eng.xin.copy_(torch.randn(B, L, eng.c.in_pad, generator=gen).to(device))
    shared.prepare_times(w.c_noise[:1])
    shared.select_time(0)
    rows.prepare_time_rows(w.c_noise)
    ms_eval = median_ms(lambda: shared.eval(False), a.repeats, sync)
    ms_rows = median_ms(lambda: rows.eval_rows(False), a.repeats, sync)
    ms_time_rows = median_ms(lambda: rows.prepare_time_rows(w.c_noise.to(device)), a.repeats, sync)
    assert shared.handoff_status() == 0 and rows.handoff_status() == 0
    res["eval"] = {"ms": round(ms_eval, 4), "launches": shared.programs["eval"].n_ops}
    res["eval_rows"] = {"ms": round(ms_rows, 4), "launches": rows.programs["eval_rows"].n_ops,
                        "time_vs_eval": round(ms_rows / ms_eval, 3), "time_rows_program_ms": round(ms_time_rows, 4)}
    # the ops of eval_rows one by one (no graph): where the time of the un-chained lowering goes
    prog, ops = rows.programs["eval_rows"], rows.c.programs["eval_rows"]
    bind = rows._bind(xin=rows.xin, out=rows.pred)
    by_kind = {}
    for _ in range(2):
        prog.run(bind, B)
    sync()
    for idx, op in enumerate(ops):
        name = rt.OP_NAMES[op.kind]
        if op.kind == rt.OP_RCONV:
            # ResNet convolutions (GroupNorm prologue, or the accumulating second half / 1x1 skip of a concatenated block) apart
            # from the resampling convolutions in patch form
            name = "k_rconv (resampling)" if (op.i[rt.R_KSRC] > 1 or op.i[rt.R_HALF_OUT] or op.i[rt.R_NB] > 1) else "k_rconv (ResNet)"
        tm = rt.EventTimer(1)
        tm.start()
        for _ in range(5):
            prog.run(bind, B, 0, idx, 1)
        tm.stop()
        us = tm.collect()[0] * 1e3 / 5
        k = by_kind.setdefault(name, {"launches": 0, "us": 0.0})
        k["launches"] += 1
        k["us"] = round(k["us"] + us, 1)
    res["eval_rows"]["ops_one_by_one"] = by_kind
    res["eval_rows"]["resnet_launch_us"] = round(sum(v["us"] for k, v in by_kind.items() if k in ("k_rconv (ResNet)", "k_resblock",
                                                                                                  "k_gn_act")), 1)

    # ---- denoise_fn with distinct sigmas: one per-row evaluation against one evaluation per value ----
    n = a.sigmas
    kd = model.diffusion.diffusion
    xs, es, ss = (x0[:n] + sig[:n].view(-1, 1, 1) * torch.randn(n, C, L, generator=gen)).to(device), emb[:n], sig[:n]
    assert len(set(ss.tolist())) == n
    ms_b = median_ms(lambda: kd.denoise_fn(xs, sigmas=ss, embedding=es, batched=True), max(a.repeats // 4, 3), sync, warmup=2)
    ms_s = median_ms(lambda: kd.denoise_fn(xs, sigmas=ss, embedding=es, batched=False), max(a.repeats // 4, 3), sync, warmup=2)
    res["denoise_distinct_sigmas"] = {"n": n, "batched_ms": round(ms_b, 3), "serial_ms": round(ms_s, 3), "speedup": round(ms_s / ms_b, 1)}

    # ---- eval_loss end to end ----
    nz = torch.randn(B, C, L, generator=gen).to(device)
    x0d = x0.to(device)
    ms_loss = median_ms(lambda: model.eval_loss(seq, x0d, device, sigmas=sig, noise=nz), a.repeats, sync)
    ms_seed = median_ms(lambda: model.eval_loss(seq, x0d, device, sigmas=sig, seed=11), a.repeats, sync)
    res["eval_loss"] = {"ms_explicit_noise": round(ms_loss, 3), "ms_counter_noise": round(ms_seed, 3),
                        "samples_per_s": round(B / (ms_seed * 1e-3))}

    # ---- the new HBM-bound kernels beside mdt_adpm2_mid ----
    KB, Cp = a.kernel_batch, 16
    x, xm, nzk = (torch.randn(KB, C, L, device=device) for _ in range(3))
    pred, xin = torch.randn(KB, L, Cp, device=device), torch.empty(KB, L, Cp, device=device)
    cf = scale_weights_rows((-1.2 + 1.2 * torch.randn(KB, generator=gen)).exp(), 0.1).packed().to(device)
    loss, ds = torch.empty(KB, device=device), torch.ones(KB, device=device)
    st, p = rt.current_stream(), rt.ptr
    calls = (
        ("mdt_adpm2_mid", 4, lambda: lib.mdt_adpm2_mid(p(x), p(pred), p(xm), p(xin), 0.5, 0.5, 1.0, -0.1, 0.7, KB, C, L, Cp, 0, st)),
        ("mdt_noise_in_rows, explicit noise", 4, lambda: lib.mdt_noise_in_rows(p(x), p(nzk), p(cf[0]), p(cf[1]), p(xm), p(xin), 0, 0, 0,
                                                                               KB, C, L, Cp, st)),
        ("mdt_noise_in_rows, counter-based noise", 3, lambda: lib.mdt_noise_in_rows(p(x), 0, p(cf[0]), p(cf[1]), p(xm), p(xin), 9, 0, 0,
                                                                                    KB, C, L, Cp, st)),
        ("mdt_precond_out_rows", 3, lambda: lib.mdt_precond_out_rows(p(x), p(pred), p(xm), p(cf[2]), p(cf[3]), KB, C, L, Cp, 0, st)),
        ("mdt_loss_rows", 3, lambda: lib.mdt_loss_rows(p(x), p(xm), p(pred), p(cf[2]), p(cf[3]), p(cf[5]), 0, p(loss), KB, C, L, Cp, st)),
        ("mdt_loss_rows, dynamic threshold", 3, lambda: lib.mdt_loss_rows(p(x), p(xm), p(pred), p(cf[2]), p(cf[3]), p(cf[5]), p(ds),
                                                                          p(loss), KB, C, L, Cp, st)))
    kern = {"batch": KB}
    for name, nbuf, call in calls:
        for _ in range(5):
            rt.check(call())
        tm = rt.EventTimer(1)
        tm.start()
        for _ in range(50):
            rt.check(call())
        tm.stop()
        us = tm.collect()[0] * 1e3 / 50
        nbytes = nbuf * KB * C * L * 4
        kern[name] = {"us_per_launch": round(us, 2), "algorithmic_mb": round(nbytes / 1e6, 1), "gb_per_s": round(nbytes / (us * 1e-6) / 1e9),
                      "hbm_peak_frac": round(nbytes / (us * 1e-6) / 1e9 / HBM_PEAK_GBS, 3)}
    base = kern["mdt_adpm2_mid"]["gb_per_s"]
    for name, _, _ in calls[1:]:
        kern[name]["vs_adpm2_mid"] = round(kern[name]["gb_per_s"] / base, 3)
    res["kernels"] = kern
    sync()
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
