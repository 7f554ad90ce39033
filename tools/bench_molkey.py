#!/usr/bin/env python3
"""What it costs to ask "which molecule is it?" of every generated row, on the GPU, inputs resident:

  (c) mol_key()                        R = 131072 rows of L = 32 positions, the mutated rows of tools/bench_smiles.py (seed 11; about half
                                       are molecules, the rest get key 0): compaction, mdt::mol_graph, mdt::mol_key, one host
                                       synchronisation per call -- beside smiles_check() on the same rows
  (g) mdt::mol_graph alone             the same rows, compacted once; op calls in a device-event interval -- beside mdt::smiles_check
  (k) mdt::mol_key alone               the graph arrays of (g)
  (f) mdt::key_flags alone             1024 keys as 128 groups of 8 against 4096 known keys, and one group of 1024
  (s) screen_tokens_diverse(vocabulary=, identity="graph") beside identity="string" at 1024 rows (forward cfg3, G = 128, N = 8,
      K = 2), interleaved

    python tools/bench_molkey.py [--rows 131072] [--length 32] [--repeats 9] [--warmup 2]      -> one JSON line

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

from bench_smiles import ALPHABET, BASES, mutated_rows  # noqa: E402  (the same rows as the validity check's measurement)

# the estimate written down before the first run: at most n * |E| ~ 400 bond steps a row at tens of cycles a step, one wave a row,
# 1024 waves resident on 256 CUs: 400 steps x 40 cycles / 2.4 GHz = 6.7 us a wave, 131072 rows / 1024 resident = 128 rounds
ESTIMATE_MOL_KEY_MS = 128 * 400 * 40 / 2.4e9 * 1e3


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=131072)
    ap.add_argument("--length", type=int, default=32)
    ap.add_argument("--screen-rows", type=int, default=1024)
    ap.add_argument("--candidates", type=int, default=8)
    ap.add_argument("--keep", type=int, default=2)
    ap.add_argument("--forward-timesteps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel-loop", type=int, default=20, help="op calls per device-event interval of (g), (k) and (f)")
    return ap.parse_args()


def main():
    a = parse()
    import torch
    from moleculediffusiontransformer_amd import NoiseSource, SmilesVocabulary, mol_key, screen_tokens_diverse, smiles_check
    from moleculediffusiontransformer_amd import ops  # noqa: F401
    from moleculediffusiontransformer_amd.synth import make_synth_model, synth_normal
    strings = mutated_rows(a.rows, width=a.length)
    vocabulary = SmilesVocabulary([None] + sorted(set("".join(BASES) + ALPHABET)))
    ids = vocabulary.encode(strings, a.length)
    if not torch.cuda.is_available():
        raise SystemExit("bench_molkey.py needs an MI355X: the kernels have no CPU fallback")
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
        once(lambda: mol_key(tok, vocabulary, device))
        once(lambda: smiles_check(tok, vocabulary, device))
    ms_c, ms_v = [], []
    for _ in range(a.repeats):
        t, (key, status, _) = once(lambda: mol_key(tok, vocabulary, device))
        ms_c.append(t)
        ms_v.append(once(lambda: smiles_check(tok, vocabulary, device))[0])
    # (g), (k), (f): the ops alone
    packed, length, _, _ = torch.ops.mdt.tokens_compact(tok.int(), 0, 1.0)
    natoms, atoms, nbonds, bonds, _, _ = torch.ops.mdt.mol_graph(packed, length, *tables)
    ms_g = [loop_ms(lambda: torch.ops.mdt.mol_graph(packed, length, *tables)) for _ in range(a.repeats)]
    ms_sc = [loop_ms(lambda: torch.ops.mdt.smiles_check(packed, length, *tables)) for _ in range(a.repeats)]
    ms_k = [loop_ms(lambda: torch.ops.mdt.mol_key(natoms, atoms, nbonds, bonds)) for _ in range(a.repeats)]
    top = -2 ** 63
    known = torch.unique(key[key != 0] ^ top)[:4096] ^ top                     # ascending as unsigned
    few = key[:a.screen_rows].contiguous()
    ms_f8 = [loop_ms(lambda: torch.ops.mdt.key_flags(few, a.candidates, known)) for _ in range(a.repeats)]
    ms_f1024 = [loop_ms(lambda: torch.ops.mdt.key_flags(few, a.screen_rows, known)) for _ in range(a.repeats)]
    molecules = int((key != 0).sum())
    steps = (natoms.long() * nbonds.long()).float()

    # (s) at the shapes of tools/bench_screen.py
    with contextlib.redirect_stdout(sys.stderr):
        inv, fwd = make_synth_model("cfg1", device), make_synth_model("cfg3", device)
    N, K = a.candidates, a.keep
    G = a.screen_rows // N
    cond = synth_normal("bench/screen/cond", (G, 12)).to(device)
    tokens = inv.sample_tokens(cond.repeat(N, 1), device, cond_scale=1.0, timesteps=2, noise=NoiseSource(seed=5))
    wide = SmilesVocabulary({i: ch for i, ch in enumerate("CNOF()=#12cno[]+-", start=1)})      # (some reading of the sampled ids)
    chain = dict(forward_timesteps=a.forward_timesteps, X_norm_factor=16.0, vocabulary=wide)

    def screen(i, identity):
        return screen_tokens_diverse(fwd, tokens, cond, device, N, K, identity=identity, forward_noise=NoiseSource(seed=900 + i), **chain)
    for w in range(max(1, a.warmup)):
        once(lambda: screen(-1 - w, "string"))
        once(lambda: screen(-1 - w, "graph"))
    ms_s = {"string": [], "graph": []}
    for i in range(a.repeats):                       # interleaved: one of each per repeat
        for identity in ms_s:
            ms_s[identity].append(once(lambda: screen(i, identity))[0])

    result = {"metric": "graph identity of token rows", "rows": a.rows, "length": a.length, "repeats": a.repeats, "warmup": a.warmup,
              "molecules": molecules, "mean_atoms_times_bonds": float(steps[key != 0].mean()) if molecules else 0.0,
              "mol_key_ms": med(ms_c), "mol_key_spread_ms": spread(ms_c),
              "smiles_check_ms": med(ms_v), "smiles_check_spread_ms": spread(ms_v),
              "mol_graph_op_ms": med(ms_g), "mol_graph_op_spread_ms": spread(ms_g),
              "smiles_check_op_ms": med(ms_sc), "smiles_check_op_spread_ms": spread(ms_sc),
              "mol_key_op_ms": med(ms_k), "mol_key_op_spread_ms": spread(ms_k),
              "mol_key_op_estimate_ms": ESTIMATE_MOL_KEY_MS, "mol_key_op_measured_over_estimate": med(ms_k) / ESTIMATE_MOL_KEY_MS,
              "key_flags_op_ms": {"128x8": med(ms_f8), "1x1024": med(ms_f1024)},
              "key_flags_op_spread_ms": {"128x8": spread(ms_f8), "1x1024": spread(ms_f1024)}, "known_keys": int(known.numel()),
              "screen_rows": a.screen_rows, "screen_tokens_ms": {k: med(v) for k, v in ms_s.items()},
              "screen_tokens_spread_ms": {k: spread(v) for k, v in ms_s.items()},
              "graph_minus_string_ms": med(ms_s["graph"]) - med(ms_s["string"]),
              "device": torch.cuda.get_device_name(device)}
    print(json.dumps(result), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
