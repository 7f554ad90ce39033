#!/usr/bin/env python3
"""What it costs to ask "how many hydrogens, and do the lower-case atoms add up?" of generated rows, on the GPU, inputs resident:

  (c) mol_hydrogens()                  R = 131072 rows of L = 32 positions, the mutated rows of tools/bench_smiles.py (about half are
                                       molecules, the rest come out all zero): compaction, mdt::mol_graph, mdt::mol_hydrogens, the
                                       widening to int64 -- beside smiles_check() and mol_fingerprint() on the same rows
  (p) mdt::mol_hydrogens alone         the graph arrays of those rows; op calls in a device-event interval -- beside mdt::mol_fp
  (v) the share of each verdict over the rows, and the most steps the reference makes on a sample of them
  (s) screen_tokens_diverse(vocabulary=) with and without kekulize=True at 1024 rows (forward cfg3, G = 128, N = 8, K = 2),
      interleaved

    python tools/bench_molh.py [--rows 131072] [--length 32] [--repeats 9] [--warmup 2]      -> one JSON line

Reported: medians and spreads (max - min) in ms, and the paper estimate of (p) beside its measurement.  There is no pass mark.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_smiles import ALPHABET, BASES, mutated_rows  # noqa: E402  (the same rows as the validity check's measurement)

# The estimate written down before the first run: instruction issue, not latency (one wave a row, 8 waves a SIMD resident, no LDS).
# A row that is no molecule leaves after its counts and one ballot: about 40 wave instructions.  A molecule: about 280 for the
# counts, the rule, the twelve ballots and the wave sum of the formula and the stores, 18 per bond entry (the sum and the 64-bit
# adjacency word), and 45 per pass of the search loop (one popcount, two or three ballots of the pick, the readlane pair, the masks);
# a try that is taken back costs a second pass.  4 cycles per wave instruction, 1024 SIMDs at 2.4 GHz.  Memory traffic (35 MB of
# graph arrays in, 16 MB out: 0.013 ms at 4 TB/s) is below that.
INSTR_NO_MOLECULE, INSTR_PER_ROW, INSTR_PER_BOND, INSTR_PER_PASS = 40, 280, 18, 45
CYCLES_PER_INSTR, SIMDS, CLOCK = 4, 1024, 2.4e9


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=131072)
    ap.add_argument("--length", type=int, default=32)
    ap.add_argument("--radius", type=int, default=2)
    ap.add_argument("--screen-rows", type=int, default=1024)
    ap.add_argument("--candidates", type=int, default=8)
    ap.add_argument("--keep", type=int, default=2)
    ap.add_argument("--forward-timesteps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel-loop", type=int, default=20, help="op calls per device-event interval of (p)")
    ap.add_argument("--estimate-rows", type=int, default=4096, help="rows whose steps the reference counts for the estimate")
    return ap.parse_args()


def estimate_ms(strings, rows):
    """-> (the paper estimate of mdt::mol_hydrogens, the most steps of a row) from the reference on a sample of the rows."""
    import molh_ref as H
    import molkey_ref as K
    instr, most = 0.0, 0
    for s in strings:
        _, _, atoms, bonds = K.graph(s)
        if not atoms:
            instr += INSTR_NO_MOLECULE
            continue
        r = H.string_hydrogens(s)
        most = max(most, r["steps"])
        passes = r["steps"] + 1 if r["verdict"] == H.OK else 2 * r["steps"] + 1      # (a search that fails takes every try back)
        instr += INSTR_PER_ROW + INSTR_PER_BOND * len(bonds) + (INSTR_PER_PASS * passes if r["wanting"] else 0)
    return 1e3 * (instr / len(strings)) * CYCLES_PER_INSTR * rows / (SIMDS * CLOCK), most


def main():
    a = parse()
    import torch
    from moleculediffusiontransformer_amd import (NoiseSource, SmilesVocabulary, mol_fingerprint, mol_hydrogens, screen_tokens_diverse,
                                                  smiles_check)
    from moleculediffusiontransformer_amd import ops  # noqa: F401
    from moleculediffusiontransformer_amd.synth import make_synth_model, synth_normal
    strings = mutated_rows(a.rows, width=a.length)
    vocabulary = SmilesVocabulary([None] + sorted(set("".join(BASES) + ALPHABET)))
    ids = vocabulary.encode(strings, a.length)
    if not torch.cuda.is_available():
        raise SystemExit("bench_molh.py needs an MI355X: the kernels have no CPU fallback")
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

    # (c): the public calls, interleaved
    legs = {"mol_hydrogens": lambda: mol_hydrogens(tok, vocabulary, device),
            "smiles_check": lambda: smiles_check(tok, vocabulary, device),
            "mol_fingerprint": lambda: mol_fingerprint(tok, vocabulary, device, a.radius)}
    for _ in range(a.warmup):
        for leg in legs.values():
            once(leg)
    ms_c = {name: [] for name in legs}
    for _ in range(a.repeats):
        for name, leg in legs.items():
            t, out = once(leg)
            ms_c[name].append(t)
            if name == "mol_hydrogens":
                verdict, status = out[2], out[4]
    # (p): the op alone, beside mdt::mol_fp
    packed, length, _, _ = torch.ops.mdt.tokens_compact(tok.int(), 0, 1.0)
    graph = torch.ops.mdt.mol_graph(packed, length, *tables)[:4]
    ms_p = [loop_ms(lambda: torch.ops.mdt.mol_hydrogens(*graph, 4096)) for _ in range(a.repeats)]
    ms_f = [loop_ms(lambda: torch.ops.mdt.mol_fp(*graph, a.radius)) for _ in range(a.repeats)]
    sample = strings[:: max(1, a.rows // a.estimate_rows)]
    estimate, most_steps = estimate_ms(sample, a.rows)
    molecules = (graph[0] > 0)
    shares = {str(v): float(((verdict == v) & molecules).float().mean()) for v in range(4)}

    # (s) at the shapes of tools/bench_screen.py
    with contextlib.redirect_stdout(sys.stderr):
        inv, fwd = make_synth_model("cfg1", device), make_synth_model("cfg3", device)
    N, K = a.candidates, a.keep
    G = a.screen_rows // N
    cond = synth_normal("bench/screen/cond", (G, 12)).to(device)
    tokens = inv.sample_tokens(cond.repeat(N, 1), device, cond_scale=1.0, timesteps=2, noise=NoiseSource(seed=5))
    wide = SmilesVocabulary({i: ch for i, ch in enumerate("CNOF()=#12cno[]+-", start=1)})      # (some reading of the sampled ids)
    chain = dict(forward_timesteps=a.forward_timesteps, X_norm_factor=16.0, vocabulary=wide)
    screens = {"plain": dict(), "kekulize": dict(kekulize=True)}

    def screen(i, leg):
        return screen_tokens_diverse(fwd, tokens, cond, device, N, K, forward_noise=NoiseSource(seed=900 + i), **screens[leg], **chain)
    for w in range(max(1, a.warmup)):
        for leg in screens:
            once(lambda: screen(-1 - w, leg))
    ms_s = {leg: [] for leg in screens}
    for i in range(a.repeats):                       # interleaved: one of each per repeat
        for leg in screens:
            t, out = once(lambda: screen(i, leg))
            ms_s[leg].append(t)
    between = med(ms_s["kekulize"]) - med(ms_s["plain"])

    result = {"metric": "implicit hydrogens and Kekule check", "rows": a.rows, "length": a.length, "repeats": a.repeats,
              "warmup": a.warmup, "rows_that_are_molecules_share": float(molecules.float().mean()),
              "rows_of_status_0_share": float((status == 0).float().mean()), "verdict_share_of_all_rows_molecules_only": shares,
              "most_steps_on_the_sample": most_steps, "estimate_rows": len(sample),
              "public_ms": {k: med(v) for k, v in ms_c.items()}, "public_spread_ms": {k: spread(v) for k, v in ms_c.items()},
              "mol_hydrogens_op_ms": med(ms_p), "mol_hydrogens_op_spread_ms": spread(ms_p),
              "mol_hydrogens_op_estimate_ms": estimate, "mol_hydrogens_op_measured_over_estimate": med(ms_p) / estimate,
              "mol_fp_op_ms": med(ms_f), "mol_fp_op_spread_ms": spread(ms_f),
              "screen_rows": a.screen_rows, "screen_tokens_ms": {k: med(v) for k, v in ms_s.items()},
              "screen_tokens_spread_ms": {k: spread(v) for k, v in ms_s.items()}, "kekulize_minus_plain_ms": between,
              "difference_inside_the_spread_of_plain": abs(between) <= spread(ms_s["plain"]),
              "device": torch.cuda.get_device_name(device)}
    print(json.dumps(result), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
