#!/usr/bin/env python3
"""What it costs to ask "how similar are two molecules?" of generated rows, on the GPU, inputs resident:

  (c) mol_fingerprint()                R = 131072 rows of L = 32 positions, the mutated rows of tools/bench_molkey.py (about half are
                                       molecules, the rest get an all-zero fingerprint): compaction, mdt::mol_graph, mdt::mol_fp, one
                                       host synchronisation per call -- beside mol_key() on the same rows
  (p) mdt::mol_fp alone                the graph arrays of those rows; op calls in a device-event interval -- beside mdt::mol_key
  (n) nearest_known_tanimoto()         the first 1024 rows against a KnownSet of the 131072 (exact repeats drop out of a KnownSet;
                                       its size is reported) -- beside nearest_known() on the same rows
  (k) mdt::fp_nearest alone            1024 fingerprints against ALL 131072 -- beside mdt::edit_nearest on the same rows
  (s) screen_tokens_diverse(vocabulary=) with and without max_similarity / max_known_similarity at 1024 rows (forward cfg3,
      G = 128, N = 8, K = 2) against 131072 known rows, interleaved

    python tools/bench_molfp.py [--rows 131072] [--length 32] [--repeats 9] [--warmup 2]      -> one JSON line

Reported: medians and spreads (max - min) in ms, and the paper estimate of (k) beside its measurement.  There is no pass mark.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_smiles import ALPHABET, BASES, mutated_rows  # noqa: E402  (the same rows as the graph key's measurement)

# the estimate written down before the first run: 32 ANDs and 32 bit counts a pair, one pair a lane-operation, 1024 SIMDs of 16
# lanes (a wave of 64 takes 4 cycles an operation) at 2.4 GHz; it ignores the compare, the loop and the scalar loads
VALU_PER_PAIR = 64
LANE_OPS_PER_SECOND = 1024 * 16 * 2.4e9


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=131072)
    ap.add_argument("--length", type=int, default=32)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--radius", type=int, default=2)
    ap.add_argument("--screen-rows", type=int, default=1024)
    ap.add_argument("--candidates", type=int, default=8)
    ap.add_argument("--keep", type=int, default=2)
    ap.add_argument("--forward-timesteps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel-loop", type=int, default=20, help="op calls per device-event interval of (p) and (k)")
    return ap.parse_args()


def main():
    a = parse()
    import numpy as np
    import torch
    from moleculediffusiontransformer_amd import (KnownSet, NoiseSource, SmilesVocabulary, mol_fingerprint, mol_key, nearest_known,
                                                  nearest_known_tanimoto, screen_tokens_diverse)
    from moleculediffusiontransformer_amd import ops  # noqa: F401
    from moleculediffusiontransformer_amd.synth import make_synth_model, synth_normal
    strings = mutated_rows(a.rows, width=a.length)
    vocabulary = SmilesVocabulary([None] + sorted(set("".join(BASES) + ALPHABET)))
    ids = vocabulary.encode(strings, a.length)
    if not torch.cuda.is_available():
        raise SystemExit("bench_molfp.py needs an MI355X: the kernels have no CPU fallback")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    tok = ids.to(device)
    tables = vocabulary.on(device)

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

    spread = lambda v: max(v) - min(v)   # noqa: E731
    med = statistics.median

    # (c): the two public calls, interleaved
    for _ in range(a.warmup):
        once(lambda: mol_fingerprint(tok, vocabulary, device, a.radius))
        once(lambda: mol_key(tok, vocabulary, device))
    ms_c, ms_key = [], []
    for _ in range(a.repeats):
        t, (fp, count, _, _) = once(lambda: mol_fingerprint(tok, vocabulary, device, a.radius))
        ms_c.append(t)
        ms_key.append(once(lambda: mol_key(tok, vocabulary, device))[0])
    # (p): the ops alone
    packed, length, _, _ = torch.ops.mdt.tokens_compact(tok.int(), 0, 1.0)
    natoms, atoms, nbonds, bonds, _, _ = torch.ops.mdt.mol_graph(packed, length, *tables)
    ms_p = [loop_ms(lambda: torch.ops.mdt.mol_fp(natoms, atoms, nbonds, bonds, a.radius)) for _ in range(a.repeats)]
    ms_pk = [loop_ms(lambda: torch.ops.mdt.mol_key(natoms, atoms, nbonds, bonds)) for _ in range(a.repeats)]
    # (n): the public searches against a KnownSet of the same rows
    known = KnownSet(ids, a.length)
    queries = tok[:a.queries]
    known.on(device)
    for _ in range(a.warmup):
        once(lambda: nearest_known_tanimoto(queries, known, vocabulary, device, a.radius))
        once(lambda: nearest_known(queries, known, device))
    ms_n, ms_e = [], []
    for _ in range(a.repeats):
        ms_n.append(once(lambda: nearest_known_tanimoto(queries, known, vocabulary, device, a.radius))[0])
        ms_e.append(once(lambda: nearest_known(queries, known, device))[0])
    # (k): the searches alone, 1024 against all rows
    qfp = fp[:a.queries].contiguous()
    ms_k = [loop_ms(lambda: torch.ops.mdt.fp_nearest(qfp, fp)) for _ in range(a.repeats)]
    qp, ql = packed[:a.queries].contiguous(), length[:a.queries].contiguous()
    ms_ke = [loop_ms(lambda: torch.ops.mdt.edit_nearest(qp, ql, packed, length), calls=max(2, a.kernel_loop // 4)) for _ in range(a.repeats)]
    pairs = float(a.queries) * a.rows
    estimate_ms = 1e3 * pairs * VALU_PER_PAIR / LANE_OPS_PER_SECOND

    # (s) at the shapes of tools/bench_screen.py
    with contextlib.redirect_stdout(sys.stderr):
        inv, fwd = make_synth_model("cfg1", device), make_synth_model("cfg3", device)
    N, K = a.candidates, a.keep
    G = a.screen_rows // N
    cond = synth_normal("bench/screen/cond", (G, 12)).to(device)
    tokens = inv.sample_tokens(cond.repeat(N, 1), device, cond_scale=1.0, timesteps=2, noise=NoiseSource(seed=5))
    wide = SmilesVocabulary({i: ch for i, ch in enumerate("CNOF()=#12cno[]+-", start=1)})      # (some reading of the sampled ids)
    rng = np.random.default_rng(17)
    rows = rng.integers(1, 16, size=(a.rows, tokens.shape[1]))
    rows[np.arange(tokens.shape[1])[None, :] >= rng.integers(8, 30, size=(a.rows, 1))] = 0
    screen_known = KnownSet(rows, tokens.shape[1])
    chain = dict(forward_timesteps=a.forward_timesteps, X_norm_factor=16.0, vocabulary=wide, known_tokens=screen_known)
    legs = {"plain": dict(), "similar": dict(max_similarity=0.7, max_known_similarity=0.7, fingerprint_radius=a.radius)}

    def screen(i, leg):
        return screen_tokens_diverse(fwd, tokens, cond, device, N, K, forward_noise=NoiseSource(seed=900 + i), **legs[leg], **chain)
    for w in range(max(1, a.warmup)):
        for leg in legs:
            once(lambda: screen(-1 - w, leg))
    ms_s = {leg: [] for leg in legs}
    for i in range(a.repeats):                       # interleaved: one of each per repeat
        for leg in legs:
            t, out = once(lambda: screen(i, leg))
            ms_s[leg].append(t)

    result = {"metric": "Tanimoto similarity on graph fingerprints", "rows": a.rows, "length": a.length, "radius": a.radius,
              "repeats": a.repeats, "warmup": a.warmup, "molecules": int((count != 0).sum()),
              "mean_bits_of_a_molecule": float(count[count != 0].float().mean()),
              "mol_fingerprint_ms": med(ms_c), "mol_fingerprint_spread_ms": spread(ms_c),
              "mol_key_ms": med(ms_key), "mol_key_spread_ms": spread(ms_key),
              "mol_fp_op_ms": med(ms_p), "mol_fp_op_spread_ms": spread(ms_p),
              "mol_key_op_ms": med(ms_pk), "mol_key_op_spread_ms": spread(ms_pk),
              "queries": a.queries, "known_set_rows": len(known),
              "nearest_known_tanimoto_ms": med(ms_n), "nearest_known_tanimoto_spread_ms": spread(ms_n),
              "nearest_known_ms": med(ms_e), "nearest_known_spread_ms": spread(ms_e),
              "fp_nearest_op_ms": med(ms_k), "fp_nearest_op_spread_ms": spread(ms_k), "fp_nearest_known_rows": a.rows,
              "fp_nearest_pairs_per_s": pairs / (med(ms_k) * 1e-3),
              "fp_nearest_op_estimate_ms": estimate_ms, "fp_nearest_op_measured_over_estimate": med(ms_k) / estimate_ms,
              "edit_nearest_op_ms": med(ms_ke), "edit_nearest_op_spread_ms": spread(ms_ke),
              "screen_rows": a.screen_rows, "screen_known_rows": len(screen_known),
              "screen_tokens_ms": {k: med(v) for k, v in ms_s.items()},
              "screen_tokens_spread_ms": {k: spread(v) for k, v in ms_s.items()},
              "similar_minus_plain_ms": med(ms_s["similar"]) - med(ms_s["plain"]),
              "device": torch.cuda.get_device_name(device)}
    print(json.dumps(result), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
