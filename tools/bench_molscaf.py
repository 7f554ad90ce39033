#!/usr/bin/env python3
"""What it costs to ask "which ring framework is it built on?" of generated rows, on the GPU, inputs resident:

  (c) mol_scaffold()                   R = 131072 rows of L = 32 positions, the mutated rows of tools/bench_smiles.py (about half are
                                       molecules, the rest come out all zero): compaction, mdt::mol_graph, mdt::mol_scaffold, the
                                       widening to int64 -- beside mol_rings() on the same rows; and scaffold_key() beside mol_key()
  (p) mdt::mol_scaffold alone          the graph arrays of those rows; op calls in a device-event interval -- beside mdt::mol_rings
                                       alone, THE YARDSTICK: the same adjacency build and ballot loops
  (v) the share of rows with flags 2 (a scaffold) and 4 (the scaffold is the whole molecule)
  (s) screen_tokens_diverse(vocabulary=, known_tokens=) with and without max_per_scaffold=1, novel_scaffold=True at 1024 rows
      (forward cfg3, G = 128, N = 8, K = 2), interleaved

    python tools/bench_molscaf.py [--rows 131072] [--length 32] [--repeats 9] [--warmup 2]      -> one JSON line
    python tools/bench_molscaf.py --estimate-only                                               -> the paper estimate, no GPU

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
# A row that is no molecule leaves after its counts, one ballot and four stores: about 45 wave instructions.  A molecule: about 130
# for the counts, the loads, the first ballot, the exocyclic ballot, the two popcounts of the kept words, the new indices of the
# lane and of its entry's two ends (a shift, a mask and two popcounts each), the two output words, the entry ballot, the seven
# stores and the flags; 16 per bond entry for the adjacency loop (decode, two compares, two 64-bit shifts and selects, the order
# test, two 64-bit ors); 11 per round of the peeling, the last one that removes nobody included (shift and test of the lane's bit,
# a 64-bit and, two popcounts and an add, compare, ballot, and-not, branch); and, for a row that was pruned, 15 per bond entry for
# the pass that sums what a kept atom lost.  4 cycles per wave instruction, 1024 SIMDs at 2.4 GHz.  Memory traffic (34 MB of graph
# arrays in, 39 MB out: 0.02 ms at 4 TB/s) is below that.
INSTR_NO_MOLECULE, INSTR_PER_ROW, INSTR_PER_BOND, INSTR_PER_ROUND, INSTR_PER_LOST_BOND = 45, 130, 16, 11, 15
CYCLES_PER_INSTR, SIMDS, CLOCK = 4, 1024, 2.4e9


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
    ap.add_argument("--kernel-loop", type=int, default=20, help="op calls per device-event interval of (p)")
    ap.add_argument("--estimate-rows", type=int, default=4096, help="rows whose peeling the reference counts for the estimate")
    ap.add_argument("--estimate-only", action="store_true", help="print the paper estimate and leave: no GPU is touched")
    return ap.parse_args()


def estimate_ms(strings, rows, mode=1):
    """-> (the paper estimate of mdt::mol_scaffold, peel rounds a molecule row, the share of molecule rows that are pruned) on a
    sample of the rows."""
    import molscaf_ref as C
    instr, rounds, pruned, molecules = 0.0, 0, 0, 0
    for s in strings:
        r = C.string_scaffold(s, mode)
        if not r["flags"]:
            instr += INSTR_NO_MOLECULE
            continue
        molecules += 1
        rounds += r["rounds"] + 1                                            # (the round that removes nobody is run as well)
        instr += INSTR_PER_ROW + INSTR_PER_BOND * r["nbonds"] + INSTR_PER_ROUND * (r["rounds"] + 1)
        if 0 < r["n"] < r["natoms"] and not mode & C.GENERIC:
            pruned += 1
            instr += INSTR_PER_LOST_BOND * r["nbonds"]
    per = max(1, molecules)
    return 1e3 * (instr / len(strings)) * CYCLES_PER_INSTR * rows / (SIMDS * CLOCK), rounds / per, pruned / per


def main():
    a = parse()
    strings = mutated_rows(a.rows, width=a.length)
    sample = strings[:: max(1, a.rows // a.estimate_rows)]
    estimate, rounds_a_molecule, pruned_share = estimate_ms(sample, a.rows)          # (before anything is measured)
    if a.estimate_only:
        print(json.dumps({"mol_scaffold_op_estimate_ms": estimate, "peel_rounds_a_molecule_row_on_the_sample": rounds_a_molecule,
                          "pruned_share_of_molecule_rows_on_the_sample": pruned_share, "estimate_rows": len(sample), "rows": a.rows}))
        return 0
    import torch
    from moleculediffusiontransformer_amd import (KnownSet, NoiseSource, SmilesVocabulary, mol_key, mol_rings, mol_scaffold,
                                                  runtime as rt, scaffold_key, screen_tokens_diverse)
    from moleculediffusiontransformer_amd import ops  # noqa: F401
    from moleculediffusiontransformer_amd.synth import make_synth_model, synth_normal
    vocabulary = SmilesVocabulary([None] + sorted(set("".join(BASES) + ALPHABET)))
    ids = vocabulary.encode(strings, a.length)
    if not torch.cuda.is_available():
        raise SystemExit("bench_molscaf.py needs an MI355X: the kernels have no CPU fallback")
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
    legs = {"mol_scaffold": lambda: mol_scaffold(tok, vocabulary, device), "mol_rings": lambda: mol_rings(tok, vocabulary, device),
            "scaffold_key": lambda: scaffold_key(tok, vocabulary, device), "mol_key": lambda: mol_key(tok, vocabulary, device)}
    for _ in range(a.warmup):
        for leg in legs.values():
            once(leg)
    ms_c = {name: [] for name in legs}
    for _ in range(a.repeats):
        for name, leg in legs.items():
            t, out = once(leg)
            ms_c[name].append(t)
            if name == "mol_scaffold":
                flags, status = out[5], out[6]
            if name == "scaffold_key":
                scaffold_keys = out[0]
            if name == "mol_key":
                keys = out[0]
    # (p): the op alone beside mdt::mol_rings (the yardstick), interleaved
    packed, length, _, _ = torch.ops.mdt.tokens_compact(tok.int(), 0, 1.0)
    graph = torch.ops.mdt.mol_graph(packed, length, *tables)[:4]
    hydrogens = torch.ops.mdt.mol_hydrogens(*graph, 4096)[0]
    kernels = {"mol_scaffold": lambda: torch.ops.mdt.mol_scaffold(*graph, rt.MOLS_EXOCYCLIC),
               "mol_scaffold_mode_0": lambda: torch.ops.mdt.mol_scaffold(*graph, 0),
               "mol_rings": lambda: torch.ops.mdt.mol_rings(*graph, hydrogens, None, None)}
    ms_p = {name: [] for name in kernels}
    for _ in range(a.repeats):
        for name, fn in kernels.items():
            ms_p[name].append(loop_ms(fn))
    distinct = lambda k: int(torch.unique(k[k != 0]).numel())   # noqa: E731

    # (s) at the shapes of tools/bench_screen.py
    with contextlib.redirect_stdout(sys.stderr):
        inv, fwd = make_synth_model("cfg1", device), make_synth_model("cfg3", device)
    N, K = a.candidates, a.keep
    G = a.screen_rows // N
    cond = synth_normal("bench/screen/cond", (G, 12)).to(device)
    tokens = inv.sample_tokens(cond.repeat(N, 1), device, cond_scale=1.0, timesteps=2, noise=NoiseSource(seed=5))
    wide = SmilesVocabulary({i: ch for i, ch in enumerate("CNOF()=#12cno[]+-", start=1)})      # (some reading of the sampled ids)
    known = KnownSet(wide.encode(["c1ccccc1", "C1CC1", "CCO", "O=C1CCCCC1"], tokens.shape[1]), tokens.shape[1])
    chain = dict(forward_timesteps=a.forward_timesteps, X_norm_factor=16.0, vocabulary=wide, known_tokens=known)
    screens = {"plain": dict(), "scaffold": dict(max_per_scaffold=1, novel_scaffold=True)}

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
    between = med(ms_s["scaffold"]) - med(ms_s["plain"])

    result = {"metric": "scaffold of the molecular graph", "rows": a.rows, "length": a.length, "repeats": a.repeats,
              "warmup": a.warmup, "rows_that_are_molecules_share": float(((flags & rt.MOLS_MOLECULE) != 0).float().mean()),
              "rows_of_status_0_share": float((status == 0).float().mean()),
              "rows_with_a_scaffold_share_flag_2": float(((flags & rt.MOLS_SCAFFOLD) != 0).float().mean()),
              "rows_whose_scaffold_is_the_whole_molecule_share_flag_4": float(((flags & rt.MOLS_WHOLE) != 0).float().mean()),
              "distinct_keys": distinct(keys), "distinct_scaffold_keys": distinct(scaffold_keys),
              "peel_rounds_a_molecule_row_on_the_sample": rounds_a_molecule,
              "pruned_share_of_molecule_rows_on_the_sample": pruned_share, "estimate_rows": len(sample),
              "public_ms": {k: med(v) for k, v in ms_c.items()}, "public_spread_ms": {k: spread(v) for k, v in ms_c.items()},
              "op_ms": {k: med(v) for k, v in ms_p.items()}, "op_spread_ms": {k: spread(v) for k, v in ms_p.items()},
              "mol_scaffold_op_over_mol_rings_op": med(ms_p["mol_scaffold"]) / med(ms_p["mol_rings"]),
              "mol_scaffold_op_estimate_ms": estimate, "mol_scaffold_op_measured_over_estimate": med(ms_p["mol_scaffold"]) / estimate,
              "screen_rows": a.screen_rows, "screen_tokens_ms": {k: med(v) for k, v in ms_s.items()},
              "screen_tokens_spread_ms": {k: spread(v) for k, v in ms_s.items()}, "scaffold_minus_plain_ms": between,
              "difference_inside_the_spread_of_the_two": abs(between) <= max(spread(ms_s["plain"]), spread(ms_s["scaffold"])),
              "device": torch.cuda.get_device_name(device)}
    print(json.dumps(result), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
