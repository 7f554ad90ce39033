#!/usr/bin/env python3
"""What it costs to ask "which bonds lie in a ring, and is the molecule inside the bounds?" of generated rows, on the GPU, inputs
resident:

  (c) mol_descriptors()                R = 131072 rows of L = 32 positions, the mutated rows of tools/bench_smiles.py (about half are
                                       molecules, the rest come out all zero): compaction, mdt::mol_graph, mdt::mol_hydrogens,
                                       mdt::mol_rings, the widening to int64 -- beside mol_hydrogens() on the same rows
  (p) mdt::mol_rings alone             the graph arrays and hydrogens of those rows; op calls in a device-event interval -- beside
                                       mdt::mol_hydrogens and mdt::mol_fp
  (v) the share of rows with at least one ring, and the ballot levels the reference counts on a sample of them
  (s) screen_tokens_diverse(vocabulary=) with and without limits=DescriptorLimits.lipinski() at 1024 rows (forward cfg3, G = 128,
      N = 8, K = 2), interleaved

    python tools/bench_molring.py [--rows 131072] [--length 32] [--repeats 9] [--warmup 2]      -> one JSON line

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
# A row that is no molecule leaves after its counts and one ballot: about 40 wave instructions.  A molecule: about 330 for the
# counts, the atom's flags, the wave sum, the eleven ballots of the weight, the sixteen descriptor selects, the bounds and the
# stores; 16 per bond entry for the 64-bit adjacency word and the two order flags; 8 per level of the component flood (and,
# compare, ballot, and-not, or, branch); when the row has a ring, 6 per entry for the second loop's loads and early exits, 14 per
# search that runs (the two masks, the start words, the three folds of the result) and 9 per level of it.  4 cycles per wave
# instruction, 1024 SIMDs at 2.4 GHz.  Memory traffic (39 MB of graph arrays and hydrogens in, 17 MB out: 0.014 ms at 4 TB/s) is
# below that.
INSTR_NO_MOLECULE, INSTR_PER_ROW, INSTR_PER_BOND, INSTR_PER_FLOOD_LEVEL = 40, 330, 16, 8
INSTR_PER_ENTRY, INSTR_PER_SEARCH, INSTR_PER_SEARCH_LEVEL = 6, 14, 9
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
    ap.add_argument("--estimate-rows", type=int, default=4096, help="rows whose levels the reference counts for the estimate")
    return ap.parse_args()


def levels_of(n, bonds):
    """-> (flood levels, searches that run, search levels) of the kernel's loops for one graph, counted on sets."""
    adj = {a: set() for a in range(n)}
    for a, b, _ in bonds:
        if a != b:
            adj[a].add(b)
            adj[b].add(a)
    seen, flood, components = set(), 0, 0
    while len(seen) < n:
        frontier = {min(set(range(n)) - seen)}
        components += 1
        while frontier:
            seen |= frontier
            flood += 1
            frontier = {y for x in frontier for y in adj[x]} - seen
    if sum(len(v) for v in adj.values()) // 2 - n + components == 0:
        return flood, 0, 0
    searches = levels = 0
    for a, b, _ in bonds:
        if a == b or len(adj[a]) == 1 or len(adj[b]) == 1:
            continue
        searches += 1
        visited = frontier = {a}
        while True:
            levels += 1
            step = {y for x in frontier for y in adj[x] if {x, y} != {a, b}} - visited
            if b in step or not step:
                break
            visited, frontier = visited | step, step
    return flood, searches, levels


def estimate_ms(strings, rows):
    """-> (the paper estimate of mdt::mol_rings, ballot levels a molecule row, the most of one row) on a sample of the rows."""
    import molkey_ref as K
    instr, ballots, molecules, most = 0.0, 0, 0, 0
    for s in strings:
        _, _, atoms, bonds = K.graph(s)
        if not atoms:
            instr += INSTR_NO_MOLECULE
            continue
        flood, searches, levels = levels_of(len(atoms), bonds)
        molecules += 1
        ballots += flood + levels
        most = max(most, flood + levels)
        instr += INSTR_PER_ROW + INSTR_PER_BOND * len(bonds) + INSTR_PER_FLOOD_LEVEL * flood
        if searches or levels:
            instr += INSTR_PER_ENTRY * len(bonds)
        instr += INSTR_PER_SEARCH * searches + INSTR_PER_SEARCH_LEVEL * levels
    return 1e3 * (instr / len(strings)) * CYCLES_PER_INSTR * rows / (SIMDS * CLOCK), ballots / max(1, molecules), most


def main():
    a = parse()
    import torch
    from moleculediffusiontransformer_amd import (DescriptorLimits, NoiseSource, SmilesVocabulary, mol_descriptors, mol_hydrogens,
                                                  screen_tokens_diverse)
    from moleculediffusiontransformer_amd import ops  # noqa: F401
    from moleculediffusiontransformer_amd.synth import make_synth_model, synth_normal
    strings = mutated_rows(a.rows, width=a.length)
    vocabulary = SmilesVocabulary([None] + sorted(set("".join(BASES) + ALPHABET)))
    ids = vocabulary.encode(strings, a.length)
    if not torch.cuda.is_available():
        raise SystemExit("bench_molring.py needs an MI355X: the kernels have no CPU fallback")
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
    legs = {"mol_descriptors": lambda: mol_descriptors(tok, vocabulary, device),
            "mol_hydrogens": lambda: mol_hydrogens(tok, vocabulary, device)}
    for _ in range(a.warmup):
        for leg in legs.values():
            once(leg)
    ms_c = {name: [] for name in legs}
    for _ in range(a.repeats):
        for name, leg in legs.items():
            t, out = once(leg)
            ms_c[name].append(t)
            if name == "mol_descriptors":
                desc, status = out[0], out[2]
    # (p): the op alone, without and with bounds, beside mdt::mol_hydrogens and mdt::mol_fp, interleaved
    packed, length, _, _ = torch.ops.mdt.tokens_compact(tok.int(), 0, 1.0)
    graph = torch.ops.mdt.mol_graph(packed, length, *tables)[:4]
    hydrogens = torch.ops.mdt.mol_hydrogens(*graph, 4096)[0]
    lo, hi = DescriptorLimits.lipinski().on(device)
    kernels = {"mol_rings": lambda: torch.ops.mdt.mol_rings(*graph, hydrogens, None, None),
               "mol_rings_bounded": lambda: torch.ops.mdt.mol_rings(*graph, hydrogens, lo, hi),
               "mol_hydrogens": lambda: torch.ops.mdt.mol_hydrogens(*graph, 4096),
               "mol_fp": lambda: torch.ops.mdt.mol_fp(*graph, a.radius)}
    ms_p = {name: [] for name in kernels}
    for _ in range(a.repeats):
        for name, fn in kernels.items():
            ms_p[name].append(loop_ms(fn))
    sample = strings[:: max(1, a.rows // a.estimate_rows)]
    estimate, levels_a_molecule, most_levels = estimate_ms(sample, a.rows)
    molecules = (graph[0] > 0)
    flagged = torch.ops.mdt.mol_rings(*graph, hydrogens, lo, hi)[3]

    # (s) at the shapes of tools/bench_screen.py
    with contextlib.redirect_stdout(sys.stderr):
        inv, fwd = make_synth_model("cfg1", device), make_synth_model("cfg3", device)
    N, K = a.candidates, a.keep
    G = a.screen_rows // N
    cond = synth_normal("bench/screen/cond", (G, 12)).to(device)
    tokens = inv.sample_tokens(cond.repeat(N, 1), device, cond_scale=1.0, timesteps=2, noise=NoiseSource(seed=5))
    wide = SmilesVocabulary({i: ch for i, ch in enumerate("CNOF()=#12cno[]+-", start=1)})      # (some reading of the sampled ids)
    chain = dict(forward_timesteps=a.forward_timesteps, X_norm_factor=16.0, vocabulary=wide)
    screens = {"plain": dict(), "limits": dict(limits=DescriptorLimits.lipinski())}

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
    between = med(ms_s["limits"]) - med(ms_s["plain"])

    result = {"metric": "ring perception and descriptors", "rows": a.rows, "length": a.length, "repeats": a.repeats,
              "warmup": a.warmup, "rows_that_are_molecules_share": float(molecules.float().mean()),
              "rows_of_status_0_share": float((status == 0).float().mean()),
              "rows_with_a_ring_share": float((desc[:, 5] > 0).float().mean()),
              "rows_outside_lipinski_share": float((flagged != 0).float().mean()),
              "ballot_levels_a_molecule_row_on_the_sample": levels_a_molecule, "most_ballot_levels_on_the_sample": most_levels,
              "estimate_rows": len(sample),
              "public_ms": {k: med(v) for k, v in ms_c.items()}, "public_spread_ms": {k: spread(v) for k, v in ms_c.items()},
              "op_ms": {k: med(v) for k, v in ms_p.items()}, "op_spread_ms": {k: spread(v) for k, v in ms_p.items()},
              "mol_rings_op_estimate_ms": estimate, "mol_rings_op_measured_over_estimate": med(ms_p["mol_rings"]) / estimate,
              "screen_rows": a.screen_rows, "screen_tokens_ms": {k: med(v) for k, v in ms_s.items()},
              "screen_tokens_spread_ms": {k: spread(v) for k, v in ms_s.items()}, "limits_minus_plain_ms": between,
              "difference_inside_the_spread_of_the_two": abs(between) <= max(spread(ms_s["plain"]), spread(ms_s["limits"])),
              "device": torch.cuda.get_device_name(device)}
    print(json.dumps(result), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
