#!/usr/bin/env python3
"""What the canonical atom order costs on generated rows, on the GPU, inputs resident:

  (k) mdt::mol_canon alone             R = 131072 rows of L = 32 positions, the mutated rows of tools/bench_molwrite.py (about half
                                       are molecules): the graph arrays of those rows; op calls in a device-event interval -- beside
                                       mdt::mol_rank alone, THE YARDSTICK: it runs n refinements a row side by side in one batch,
                                       where the search runs one batch per node that is no leaf and one per component
  (c) mol_respell(canonical=True)      compaction, mdt::mol_graph, mdt::mol_rank, mdt::mol_canon, the select, mdt::mol_write, the
                                       widening to int64 -- beside mol_respell() on the same rows
  (v) the share of rows with each flag (1 canonical, 2 undecided, 0 no molecule), and of the canonical rows the nodes of the search:
      mean, max, the share with one node

    python tools/bench_molcanon.py [--rows 131072] [--length 32] [--repeats 9] [--warmup 2]      -> one JSON line
    python tools/bench_molcanon.py --estimate-only                                               -> the paper estimate, no GPU

Reported: medians and spreads (max - min) in ms, and the paper estimate of (k) beside its measurement.  There is no pass mark.
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

from bench_smiles import ALPHABET, BASES, mutated_rows  # noqa: E402  (the same rows as the writer's measurement)

# The estimate written down before the first run: instruction issue, not latency (one wave a row), with the terms of
# tools/bench_molwrite.py for the refinement.  A row that is no molecule leaves after its counts, one ballot and four stores: about
# 30 wave instructions.  A molecule: 260 a row (loads, the output, the rank and offsets of one component), 30 an entry (16 for the
# adjacency, 14 for the twin key), 14 an atom for the twin word, 60 a component and 6 a level for its flood and its bookkeeping, 40 a
# pair of components for their compare.  A BATCH -- the children of one node refined side by side, or the root of a component -- is
# mdt::mol_rank's refinement (50 an atom to seed, a round 64 an entry and 48 an atom) plus the target: 12 an atom, and 6 an atom for
# each class it has to collect, taken as half the atoms, plus 60 for the descent.  A LEAF: 8 an atom for its position, 8 an entry for
# its rank, 90 for the certificate line, the compare and the copy.  4 cycles per wave instruction, 1024 SIMDs at 2.4 GHz.  Memory
# traffic (34 MB in, 67 MB out: 0.03 ms at 4 TB/s) is not added.
K_NO_MOLECULE, K_PER_ROW, K_PER_ENTRY, K_PER_ATOM, K_PER_COMPONENT, K_PER_LEVEL, K_PER_PAIR = 30, 260, 30, 14, 60, 6, 40
K_SEED, K_PER_ROUND_ENTRY, K_PER_ROUND_ATOM, K_TARGET_ATOM, K_TARGET_CLASS_ATOM, K_DESCENT = 50, 64, 48, 12, 6, 60
K_LEAF, K_LEAF_ATOM, K_LEAF_ENTRY = 90, 8, 8
CYCLES_PER_INSTR, SIMDS, CLOCK = 4, 1024, 2.4e9


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=131072)
    ap.add_argument("--length", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel-loop", type=int, default=20, help="op calls per device-event interval of (k)")
    ap.add_argument("--estimate-rows", type=int, default=4096, help="rows the reference searches for the estimate")
    ap.add_argument("--estimate-only", action="store_true", help="print the paper estimate and leave: no GPU is touched")
    return ap.parse_args()


def estimate_ms(strings, rows):
    """-> (the paper estimate of mdt::mol_canon in ms, nodes a molecule row, batches a molecule row) on a sample of the rows."""
    import molcanon_ref as Q
    import molkey_ref as K
    total = 0.0
    molecules = nodes_seen = batches_seen = 0
    for s in strings:
        _, _, atoms, bonds = K.graph(s)
        n, nb = len(atoms), len(bonds)
        if n == 0:
            total += K_NO_MOLECULE
            continue
        out = Q.canon(n, atoms, nb, bonds, 64)
        parts = len(Q.components(n, bonds))
        batches = out["nodes"] - out["leaves"] + parts                        # every node that is no leaf, and every root
        molecules, nodes_seen, batches_seen = molecules + 1, nodes_seen + out["nodes"], batches_seen + batches
        total += K_PER_ROW + K_PER_ENTRY * nb + K_PER_ATOM * n + parts * K_PER_COMPONENT + K_PER_LEVEL * n + K_PER_PAIR * parts * (parts - 1) // 2
        total += batches * (K_SEED * n + n * (K_PER_ROUND_ENTRY * nb + K_PER_ROUND_ATOM * n) + K_TARGET_ATOM * n +
                            K_TARGET_CLASS_ATOM * n * n // 2 + K_DESCENT)
        total += out["leaves"] * (K_LEAF + K_LEAF_ATOM * n + K_LEAF_ENTRY * nb)
    to_ms = lambda instr: 1e3 * (instr / len(strings)) * CYCLES_PER_INSTR * rows / (SIMDS * CLOCK)   # noqa: E731
    per = max(1, molecules)
    return to_ms(total), nodes_seen / per, batches_seen / per


def main():
    a = parse()
    strings = mutated_rows(a.rows, width=a.length)
    sample = strings[:: max(1, a.rows // a.estimate_rows)]
    canon_estimate, nodes_a_molecule, batches_a_molecule = estimate_ms(sample, a.rows)    # (before anything is measured)
    if a.estimate_only:
        print(json.dumps({"mol_canon_op_estimate_ms": canon_estimate, "nodes_a_molecule_row_on_the_sample": nodes_a_molecule,
                          "batches_a_molecule_row_on_the_sample": batches_a_molecule, "estimate_rows": len(sample), "rows": a.rows}))
        return 0
    import torch
    from moleculediffusiontransformer_amd import SmilesVocabulary, mol_respell, runtime as rt
    from moleculediffusiontransformer_amd import ops  # noqa: F401
    vocabulary = SmilesVocabulary([None] + sorted(set("".join(BASES) + ALPHABET)))
    ids = vocabulary.encode(strings, a.length)
    if not torch.cuda.is_available():
        raise SystemExit("bench_molcanon.py needs an MI355X: the kernels have no CPU fallback")
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
    legs = {"mol_respell_canonical": lambda: mol_respell(tok, vocabulary, device, canonical=True),
            "mol_respell": lambda: mol_respell(tok, vocabulary, device)}
    for _ in range(a.warmup):
        for leg in legs.values():
            once(leg)
    ms_c = {name: [] for name in legs}
    written = {}
    for _ in range(a.repeats):
        for name, leg in legs.items():
            t, out = once(leg)
            ms_c[name].append(t)
            written[name] = out[0]
    # (k): the op alone beside its yardstick, interleaved
    packed, length, _, _ = torch.ops.mdt.tokens_compact(tok.int(), 0, 1.0)
    graph = torch.ops.mdt.mol_graph(packed, length, *tables)[:4]
    _, _, _, nodes, flags = torch.ops.mdt.mol_canon(*graph)
    kernels = {"mol_canon": lambda: torch.ops.mdt.mol_canon(*graph), "mol_rank": lambda: torch.ops.mdt.mol_rank(*graph)}
    ms_p = {name: [] for name in kernels}
    for _ in range(a.repeats):
        for name, fn in kernels.items():
            ms_p[name].append(loop_ms(fn))
    rows_of = lambda t: int(torch.unique(t[(t != 0).any(dim=1)], dim=0).shape[0])   # noqa: E731
    share = lambda f: float((flags == f).float().mean())   # noqa: E731
    decided = nodes[flags == rt.MOLC_CANONICAL].float()
    result = {"metric": "canonical atom order of graph rows", "rows": a.rows, "length": a.length, "repeats": a.repeats, "warmup": a.warmup,
              "flag_share": {"0_no_molecule": share(0), "1_canonical": share(rt.MOLC_CANONICAL), "2_undecided": share(rt.MOLC_UNDECIDED)},
              "nodes_of_canonical_rows": {"mean": float(decided.mean()), "max": int(decided.max()), "share_with_1": float((decided == 1).float().mean())},
              "distinct_written_rows": {k: rows_of(v) for k, v in written.items()},
              "rows_that_differ": int((written["mol_respell_canonical"] != written["mol_respell"]).any(dim=1).sum()),
              "nodes_a_molecule_row_on_the_sample": nodes_a_molecule, "batches_a_molecule_row_on_the_sample": batches_a_molecule,
              "estimate_rows": len(sample),
              "public_ms": {k: med(v) for k, v in ms_c.items()}, "public_spread_ms": {k: spread(v) for k, v in ms_c.items()},
              "op_ms": {k: med(v) for k, v in ms_p.items()}, "op_spread_ms": {k: spread(v) for k, v in ms_p.items()},
              "mol_canon_op_over_mol_rank_op": med(ms_p["mol_canon"]) / med(ms_p["mol_rank"]),
              "mol_canon_op_estimate_ms": canon_estimate, "mol_canon_op_measured_over_estimate": med(ms_p["mol_canon"]) / canon_estimate,
              "device": torch.cuda.get_device_name(device)}
    print(json.dumps(result), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
