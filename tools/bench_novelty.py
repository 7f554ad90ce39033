#!/usr/bin/env python3
"""What it costs to ask "how far from the known set?" instead of "is it in the known set?", on the GPU, inputs resident:

  (n) nearest_known()                 R = 1024 query rows (8 candidates x 128 targets) of L = 32 positions, ids below 22, against a
                                      known set of M = 131072 random rows of 8 to 29 ids: compaction, the id check (one host
                                      synchronisation) and mdt::edit_nearest
  (k) mdt::edit_nearest alone         the same rows, one op call per device-event interval entry
  (m) mdt::screen_select alone        the exact-membership lookup of the same rows in the same known set (8 candidates per group)
  (s) screen_tokens() beside screen_tokens_diverse(min_distance=3) at the shapes of tools/bench_screen.py (forward cfg3 at 100
      timesteps, G = 128, N = 8, K = 2), interleaved

    python tools/bench_novelty.py [--rows 1024] [--known 131072] [--length 32] [--repeats 9] [--warmup 2]      -> one JSON line

Reported: medians and spreads (max - min) in ms, pairs per second and cells of the dynamic programme per second (pairs x mean
query length x mean known length).  "paper_estimate_ms" is NOT a measurement: lane-operations of the recurrence over the lane
throughput of the device (the constants below), quoted only beside the measured time and their ratio.  There is no pass mark.
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

# the paper estimate: 32-bit lane operations per text symbol of one pair (about 15 64-bit operations, two halves each) over
# compute units x SIMDs x 16 lanes x clock of an MI355X
LANE_OPS_PER_SYMBOL = 30
LANES_PER_SECOND = 256 * 4 * 16 * 2.4e9


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--known", type=int, default=131072)
    ap.add_argument("--length", type=int, default=32)
    ap.add_argument("--candidates", type=int, default=8)
    ap.add_argument("--keep", type=int, default=2)
    ap.add_argument("--forward-timesteps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel-loop", type=int, default=20, help="op calls per device-event interval of (k) and (m)")
    return ap.parse_args()


def random_rows(rng, rows, length, lo=8, hi=29, top=22):
    """(rows, length) ids in [1, top) in the first n positions, n uniform in [lo, min(hi, length)]."""
    import numpy as np
    n = rng.integers(lo, min(hi, length) + 1, rows)
    ids = rng.integers(1, top, (rows, length))
    return ids * (np.arange(length)[None, :] < n[:, None]), n


def main():
    a = parse()
    import numpy as np
    import torch
    from moleculediffusiontransformer_amd import (KnownSet, NoiseSource, nearest_known, screen_tokens, screen_tokens_diverse)
    from moleculediffusiontransformer_amd import ops  # noqa: F401
    from moleculediffusiontransformer_amd.synth import make_synth_model, synth_normal
    rng = np.random.default_rng(2024)
    queries, qn = random_rows(rng, a.rows, a.length)
    known_rows, _ = random_rows(rng, a.known, a.length)
    known = KnownSet(known_rows, a.length)
    M = len(known)
    pairs = a.rows * M
    cells = pairs * float(qn.mean()) * float(known.lengths.mean())
    estimate_ms = 1e3 * pairs * float(known.lengths.mean()) * LANE_OPS_PER_SYMBOL / LANES_PER_SECOND
    if not torch.cuda.is_available():
        raise SystemExit("bench_novelty.py needs an MI355X: the edit-distance path has no CPU fallback")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    tok = torch.from_numpy(queries).to(device)
    known.on(device)

    def once(leg):
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        out = leg()
        torch.cuda.synchronize(device)
        return 1e3 * (time.perf_counter() - t0), out

    def loop_ms(fn, calls=a.kernel_loop):
        fn()
        torch.cuda.synchronize(device)
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(calls):
            fn()
        stop.record()
        torch.cuda.synchronize(device)
        return start.elapsed_time(stop) / calls

    # (n), (k), (m)
    for _ in range(a.warmup):
        once(lambda: nearest_known(tok, known, device))
    ms_n = []
    for _ in range(a.repeats):
        t, (dist, index) = once(lambda: nearest_known(tok, known, device))
        ms_n.append(t)
    packed, length, key, _ = torch.ops.mdt.tokens_compact(tok, 0, 1.0)
    kk, kp, kl = known.on(device)
    ms_k = [loop_ms(lambda: torch.ops.mdt.edit_nearest(packed, length, kp, kl)) for _ in range(a.repeats)]
    N, K = a.candidates, a.keep
    score = torch.rand(a.rows, device=device)
    ms_m = [loop_ms(lambda: torch.ops.mdt.screen_select(score, key, packed, length, N, K, kk, kp, kl)) for _ in range(a.repeats)]
    med_n, med_k, med_m = statistics.median(ms_n), statistics.median(ms_k), statistics.median(ms_m)

    # (s) at the shapes of tools/bench_screen.py
    with contextlib.redirect_stdout(sys.stderr):
        inv, fwd = make_synth_model("cfg1", device), make_synth_model("cfg3", device)
    G = a.rows // N
    cond = synth_normal("bench/screen/cond", (G, 12)).to(device)
    tokens = inv.sample_tokens(cond.repeat(N, 1), device, cond_scale=1.0, timesteps=2, noise=NoiseSource(seed=5))
    chain = dict(forward_timesteps=a.forward_timesteps, X_norm_factor=16.0)

    def plain(i):
        return screen_tokens(fwd, tokens, cond, device, N, K, forward_noise=NoiseSource(seed=900 + i), **chain)

    def diverse(i):
        return screen_tokens_diverse(fwd, tokens, cond, device, N, K, min_distance=3, forward_noise=NoiseSource(seed=900 + i), **chain)
    for w in range(max(1, a.warmup)):
        once(lambda: plain(-1 - w))
        once(lambda: diverse(-1 - w))
    ms_s = {"min_distance_1": [], "min_distance_3": []}
    close = 0
    for i in range(a.repeats):                       # interleaved: one of each per repeat
        ms_s["min_distance_1"].append(once(lambda: plain(i))[0])
        t, out = once(lambda: diverse(i))
        ms_s["min_distance_3"].append(t)
        close = int(((out.status & 16) != 0).sum())
    med_s = {k: statistics.median(v) for k, v in ms_s.items()}

    spread = lambda v: max(v) - min(v)
    result = {"metric": "nearest known molecule by edit distance", "rows": a.rows, "known": M, "length": a.length,
              "mean_query_length": float(qn.mean()), "mean_known_length": float(known.lengths.mean()),
              "repeats": a.repeats, "warmup": a.warmup,
              "nearest_known_ms": med_n, "nearest_known_spread_ms": spread(ms_n),
              "edit_nearest_op_ms": med_k, "edit_nearest_op_spread_ms": spread(ms_k),
              "pairs_per_s": pairs / (1e-3 * med_k), "cells_per_s": cells / (1e-3 * med_k),
              "paper_estimate_ms": estimate_ms, "paper_estimate_is": "unmeasured: lane operations over lane throughput",
              "measured_over_estimate": med_k / estimate_ms,
              "screen_select_exact_ms": med_m, "screen_select_exact_spread_ms": spread(ms_m),
              "how_far_over_whether": med_k / med_m,
              "max_distance_found": int(dist.max()), "min_distance_found": int(dist.min()),
              "screen_tokens_ms": med_s, "screen_tokens_spread_ms": {k: spread(v) for k, v in ms_s.items()},
              "min_distance_3_minus_1_ms": med_s["min_distance_3"] - med_s["min_distance_1"], "close_rows_last_repeat": close,
              "device": torch.cuda.get_device_name(device)}
    print(json.dumps(result), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
