#!/usr/bin/env python3
"""What it costs to spell generated rows under one spelling, on the GPU, inputs resident:

  (c) mol_respell()                    R = 131072 rows of L = 32 positions, the mutated rows of tools/bench_smiles.py (about half are
                                       molecules, the rest come out all zero): compaction, mdt::mol_graph, mdt::mol_rank,
                                       mdt::mol_write, the widening to int64 -- beside mol_key() on the same rows
  (r) mdt::mol_rank alone              the graph arrays of those rows; op calls in a device-event interval -- beside mdt::mol_key
                                       alone, THE YARDSTICK: the same refinement, plus a flood and a column read
  (w) mdt::mol_write alone             with the priority of (r) and without one -- beside mdt::mol_graph alone, THE YARDSTICK: both
                                       pay a serial walk per row and R * L words of traffic
  (v) the share of rows with each flag (1 written, 2 too long for the input's width, 4 no vocabulary, 8 not writable, 0 no molecule)

    python tools/bench_molwrite.py [--rows 131072] [--length 32] [--repeats 9] [--warmup 2]      -> one JSON line
    python tools/bench_molwrite.py --estimate-only                                               -> the paper estimates, no GPU

Reported: medians and spreads (max - min) in ms, and the paper estimates of (r) and (w) beside their measurements.  There is no
pass mark.
"""
import argparse
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

# The estimates written down before the first run: instruction issue, not latency (one wave a row, 8 waves a SIMD resident).
# mdt::mol_write.  A row that is no molecule leaves after its counts, one ballot and six stores: about 50 wave instructions.  A
# molecule: about 400 for the counts, the loads, the checks, the two prefix sums (6 shuffles and selects each), the LDS lines and the
# output; 56 per bond entry for the three passes over the entries (14 for the pairs named twice, 16 for the rank space with its two
# readlanes, 26 for the seq space with the three order planes); 70 per atom (10 for its turn in the rank compares, 6 in the
# children loop, 2 steps of pass 1 at 22 each -- a readlane pair, and-not, find-first-set, selects, branch --, 10 in the number walk);
# 60 per ring closure (its two turns in the number walk with their readlanes and popcounts, and its number in both token passes);
# and, because the lanes emit their atoms side by side, 28 per token of the row's LONGEST atom (two passes of about 14: class_id
# load, test, LDS store, count).  mdt::mol_rank: mdt::mol_key's refinement -- 50 per atom to seed, per round 64 per entry (two LDS
# loads, two adds and mixes of about 20, two LDS read-modify-writes) and 48 per atom (two mixes, two stores), 24 per atom for H --
# plus 60 for the adjacency, and 40 + 6 per level for each component's flood, minimum and column read.  4 cycles per wave
# instruction, 1024 SIMDs at 2.4 GHz.  Memory traffic (34 MB of graph arrays and 34 MB of priority in, 21 MB out: 0.02 ms at
# 4 TB/s) is below the issue estimate of (w) and far below that of (r).
W_NO_MOLECULE, W_PER_ROW, W_PER_BOND, W_PER_ATOM, W_PER_CLOSURE, W_PER_TOKEN_OF_LONGEST_ATOM = 50, 400, 56, 70, 60, 28
R_NO_MOLECULE, R_PER_ROW, R_SEED, R_PER_ROUND_ENTRY, R_PER_ROUND_ATOM, R_H, R_PER_COMPONENT, R_PER_LEVEL = 20, 60, 50, 64, 48, 24, 40, 6
CYCLES_PER_INSTR, SIMDS, CLOCK = 4, 1024, 2.4e9


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=131072)
    ap.add_argument("--length", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel-loop", type=int, default=20, help="op calls per device-event interval of (r) and (w)")
    ap.add_argument("--estimate-rows", type=int, default=4096, help="rows the reference walks for the estimates")
    ap.add_argument("--estimate-only", action="store_true", help="print the paper estimates and leave: no GPU is touched")
    return ap.parse_args()


def estimate_ms(strings, rows):
    """-> (the paper estimates of mdt::mol_write and of mdt::mol_rank in ms, atoms a molecule row, closures a molecule row) on a
    sample of the rows."""
    import molkey_ref as K
    import molwrite_ref as W
    write = rank = 0.0
    molecules = atoms_seen = closures_seen = 0
    for s in strings:
        _, _, atoms, bonds = K.graph(s)
        n, nb = len(atoms), len(bonds)
        if n == 0:
            write += W_NO_MOLECULE
            rank += R_NO_MOLECULE
            continue
        out = W.write_arrays(n, atoms, nb, bonds, None, W.ASCII_CLASS_ID, 128)
        comp = W.components(n, bonds)
        parts = len(set(comp))
        closures = nb - n + parts
        longest = max([out["owners"].count(1 + a) for a in range(n)] + [1])
        molecules, atoms_seen, closures_seen = molecules + 1, atoms_seen + n, closures_seen + closures
        write += W_PER_ROW + W_PER_BOND * nb + W_PER_ATOM * n + W_PER_CLOSURE * closures + W_PER_TOKEN_OF_LONGEST_ATOM * longest
        rank += (R_PER_ROW + R_SEED * n + n * (R_PER_ROUND_ENTRY * nb + R_PER_ROUND_ATOM * n) + R_H * n + 16 * nb +
                 parts * R_PER_COMPONENT + R_PER_LEVEL * n)
    to_ms = lambda instr: 1e3 * (instr / len(strings)) * CYCLES_PER_INSTR * rows / (SIMDS * CLOCK)   # noqa: E731
    per = max(1, molecules)
    return to_ms(write), to_ms(rank), atoms_seen / per, closures_seen / per


def main():
    a = parse()
    strings = mutated_rows(a.rows, width=a.length)
    sample = strings[:: max(1, a.rows // a.estimate_rows)]
    write_estimate, rank_estimate, atoms_a_molecule, closures_a_molecule = estimate_ms(sample, a.rows)    # (before anything is measured)
    if a.estimate_only:
        print(json.dumps({"mol_write_op_estimate_ms": write_estimate, "mol_rank_op_estimate_ms": rank_estimate,
                          "atoms_a_molecule_row_on_the_sample": atoms_a_molecule, "closures_a_molecule_row_on_the_sample": closures_a_molecule,
                          "estimate_rows": len(sample), "rows": a.rows}))
        return 0
    import torch
    from moleculediffusiontransformer_amd import SmilesVocabulary, mol_key, mol_respell, runtime as rt
    from moleculediffusiontransformer_amd import ops  # noqa: F401
    vocabulary = SmilesVocabulary([None] + sorted(set("".join(BASES) + ALPHABET)))
    ids = vocabulary.encode(strings, a.length)
    if not torch.cuda.is_available():
        raise SystemExit("bench_molwrite.py needs an MI355X: the kernels have no CPU fallback")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    tok = ids.to(device)
    tables = vocabulary.on(device)
    class_id = vocabulary.class_id_on(device)

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
    legs = {"mol_respell": lambda: mol_respell(tok, vocabulary, device), "mol_respell_as_numbered": lambda: mol_respell(tok, vocabulary, device, invariant=False),
            "mol_key": lambda: mol_key(tok, vocabulary, device)}
    for _ in range(a.warmup):
        for leg in legs.values():
            once(leg)
    ms_c = {name: [] for name in legs}
    for _ in range(a.repeats):
        for name, leg in legs.items():
            t, out = once(leg)
            ms_c[name].append(t)
            if name == "mol_respell":
                written, flags = out[0], out[1]
            if name == "mol_key":
                keys = out[0]
    # (r), (w): the ops alone beside their yardsticks, interleaved
    packed, length, _, _ = torch.ops.mdt.tokens_compact(tok.int(), 0, 1.0)
    graph = torch.ops.mdt.mol_graph(packed, length, *tables)[:4]
    priority = torch.ops.mdt.mol_rank(*graph)
    kernels = {"mol_rank": lambda: torch.ops.mdt.mol_rank(*graph), "mol_key": lambda: torch.ops.mdt.mol_key(*graph),
               "mol_write": lambda: torch.ops.mdt.mol_write(*graph, priority, class_id, a.length),
               "mol_write_as_numbered": lambda: torch.ops.mdt.mol_write(*graph, None, class_id, a.length),
               "mol_graph": lambda: torch.ops.mdt.mol_graph(packed, length, *tables)}
    ms_p = {name: [] for name in kernels}
    for _ in range(a.repeats):
        for name, fn in kernels.items():
            ms_p[name].append(loop_ms(fn))
    rows_of = lambda t: int(torch.unique(t[(t != 0).any(dim=1)], dim=0).shape[0])   # noqa: E731
    share = lambda f: float((flags == f).float().mean())   # noqa: E731
    result = {"metric": "graph rows written as SMILES tokens", "rows": a.rows, "length": a.length, "repeats": a.repeats, "warmup": a.warmup,
              "flag_share": {"0_no_molecule": share(0), "1_written": share(rt.MOLW_WRITTEN), "2_too_long": share(rt.MOLW_NO_FIT),
                             "4_no_vocabulary": share(rt.MOLW_NO_VOCABULARY), "8_not_writable": share(rt.MOLW_NOT_WRITABLE)},
              "distinct_keys": int(torch.unique(keys[keys != 0]).numel()), "distinct_written_rows": rows_of(written),
              "atoms_a_molecule_row_on_the_sample": atoms_a_molecule, "closures_a_molecule_row_on_the_sample": closures_a_molecule,
              "estimate_rows": len(sample),
              "public_ms": {k: med(v) for k, v in ms_c.items()}, "public_spread_ms": {k: spread(v) for k, v in ms_c.items()},
              "op_ms": {k: med(v) for k, v in ms_p.items()}, "op_spread_ms": {k: spread(v) for k, v in ms_p.items()},
              "mol_rank_op_over_mol_key_op": med(ms_p["mol_rank"]) / med(ms_p["mol_key"]),
              "mol_write_op_over_mol_graph_op": med(ms_p["mol_write"]) / med(ms_p["mol_graph"]),
              "mol_rank_op_estimate_ms": rank_estimate, "mol_rank_op_measured_over_estimate": med(ms_p["mol_rank"]) / rank_estimate,
              "mol_write_op_estimate_ms": write_estimate, "mol_write_op_measured_over_estimate": med(ms_p["mol_write"]) / write_estimate,
              "device": torch.cuda.get_device_name(device)}
    print(json.dumps(result), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
