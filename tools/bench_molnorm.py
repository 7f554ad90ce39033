#!/usr/bin/env python3
"""What it costs to ask "which molecule is it, whatever the spelling of its rings and hydrogens?" of generated rows, on the GPU,
inputs resident:

  (c) mol_normalize()                  R = 131072 rows of L = 32 positions, the mutated rows of tools/bench_smiles.py (about half are
                                       molecules, the rest come out all zero): compaction, mdt::mol_graph, mdt::mol_hydrogens,
                                       mdt::mol_rings, mdt::mol_normalize, the widening to int64 -- beside mol_rings() on the same
                                       rows; and mol_key(normalize=True) beside mol_key()
  (p) mdt::mol_normalize alone         the graph arrays, hydrogens, Kekule structure and ring sizes of those rows; op calls in a
                                       device-event interval -- beside mdt::mol_rings and mdt::mol_hydrogens, THE YARDSTICK BEING
                                       mdt::mol_rings: it runs the same per-entry searches
  (v) the share of rows with flags 2 (an aromatic ring) and 4 (something differs from what was written)
  (s) screen_tokens_diverse(vocabulary=, identity="graph") with and without normalize=True at 1024 rows (forward cfg3, G = 128,
      N = 8, K = 2), interleaved

    python tools/bench_molnorm.py [--rows 131072] [--length 32] [--repeats 9] [--warmup 2]      -> one JSON line

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
# A row that is no molecule leaves after its counts and one ballot, a row without a Kekule structure after one more load and two
# stores: about 40 / 55 wave instructions.  A molecule: about 150 for the counts, the loads, the partner's descriptor, the pi rule
# (a dozen selects), the three ballots, the entry's own Kekule order, the output words, the change ballot and the stores; 24 per
# bond entry for the per-atom loop (decode, Kekule order, the 64-bit adjacency word, the five counts).  For every entry that is
# searched -- a ring bond between eligible atoms: 22 to start (the entry's word, the two masks, the start words), 11 per level of
# the search (and, compare, ballot, and-not, the level select, two tests, or, branch), 8 per level of each of the two walks back
# (three tests, ballot, find-bit, shift, or, branch), 22 for the two Hueckel tests and the marking.  A ring of size r has r - 1
# search levels and r - 2 walk levels a walk.  4 cycles per wave instruction, 1024 SIMDs at 2.4 GHz.  Memory traffic (47 MB of graph
# arrays, hydrogens, partners and ring sizes in, 34 MB out: 0.02 ms at 4 TB/s) is below that.
INSTR_NO_MOLECULE, INSTR_NO_KEKULE, INSTR_PER_ROW, INSTR_PER_BOND = 40, 55, 150, 24
INSTR_PER_SEARCH, INSTR_PER_SEARCH_LEVEL, INSTR_PER_WALK_LEVEL, INSTR_PER_JUDGEMENT = 22, 11, 8, 22
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
    ap.add_argument("--estimate-rows", type=int, default=4096, help="rows whose searches the reference counts for the estimate")
    return ap.parse_args()


def estimate_ms(strings, rows):
    """-> (the paper estimate of mdt::mol_normalize, searches a molecule row, ballots a molecule row) on a sample of the rows."""
    import molh_ref as H
    import molkey_ref as K
    import molnorm_ref as N
    import molring_ref as R
    instr, searches, ballots, molecules = 0.0, 0, 0, 0
    for s in strings:
        _, _, atoms, bonds = K.graph(s)
        if not atoms:
            instr += INSTR_NO_MOLECULE
            continue
        h = H.string_hydrogens(s)
        if h["verdict"] != 0:
            instr += INSTR_NO_KEKULE
            continue
        molecules += 1
        instr += INSTR_PER_ROW + INSTR_PER_BOND * len(bonds)
        ring = R.string_rings(s)["bond_ring"]
        p = N.pi_electrons(len(atoms), atoms, bonds, N.kekule_orders(bonds, h["partner"]), h["hydrogens"], ring)
        for e, (a, b, _) in enumerate(bonds):
            if a == b or not ring[e] or p[a] is None or p[b] is None:
                continue
            searches += 1
            ballots += ring[e] - 1 + 2 * (ring[e] - 2)
            instr += INSTR_PER_SEARCH + INSTR_PER_SEARCH_LEVEL * (ring[e] - 1) + 2 * INSTR_PER_WALK_LEVEL * (ring[e] - 2) + INSTR_PER_JUDGEMENT
    per = max(1, molecules)
    return 1e3 * (instr / len(strings)) * CYCLES_PER_INSTR * rows / (SIMDS * CLOCK), searches / per, ballots / per


def main():
    a = parse()
    import torch
    from moleculediffusiontransformer_amd import (NoiseSource, SmilesVocabulary, mol_key, mol_normalize, mol_rings, runtime as rt,
                                                  screen_tokens_diverse)
    from moleculediffusiontransformer_amd import ops  # noqa: F401
    from moleculediffusiontransformer_amd.synth import make_synth_model, synth_normal
    strings = mutated_rows(a.rows, width=a.length)
    vocabulary = SmilesVocabulary([None] + sorted(set("".join(BASES) + ALPHABET)))
    ids = vocabulary.encode(strings, a.length)
    if not torch.cuda.is_available():
        raise SystemExit("bench_molnorm.py needs an MI355X: the kernels have no CPU fallback")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    tok = ids.to(device)
    tables = vocabulary.on(device)
    sample = strings[:: max(1, a.rows // a.estimate_rows)]
    estimate, searches_a_molecule, ballots_a_molecule = estimate_ms(sample, a.rows)      # (before anything is measured)

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
    legs = {"mol_normalize": lambda: mol_normalize(tok, vocabulary, device), "mol_rings": lambda: mol_rings(tok, vocabulary, device),
            "mol_key_normalized": lambda: mol_key(tok, vocabulary, device, normalize=True),
            "mol_key": lambda: mol_key(tok, vocabulary, device)}
    for _ in range(a.warmup):
        for leg in legs.values():
            once(leg)
    ms_c = {name: [] for name in legs}
    for _ in range(a.repeats):
        for name, leg in legs.items():
            t, out = once(leg)
            ms_c[name].append(t)
            if name == "mol_normalize":
                flags, status = out[4], out[6]
            if name == "mol_key_normalized":
                normal_keys = out[0]
            if name == "mol_key":
                keys = out[0]
    # (p): the op alone beside mdt::mol_rings (the yardstick) and mdt::mol_hydrogens, interleaved
    packed, length, _, _ = torch.ops.mdt.tokens_compact(tok.int(), 0, 1.0)
    graph = torch.ops.mdt.mol_graph(packed, length, *tables)[:4]
    hydrogens, partner, verdict, _, _ = torch.ops.mdt.mol_hydrogens(*graph, 4096)
    bond_ring = torch.ops.mdt.mol_rings(*graph, hydrogens, None, None)[0]
    kernels = {"mol_normalize": lambda: torch.ops.mdt.mol_normalize(*graph, hydrogens, partner, verdict, bond_ring),
               "mol_rings": lambda: torch.ops.mdt.mol_rings(*graph, hydrogens, None, None),
               "mol_hydrogens": lambda: torch.ops.mdt.mol_hydrogens(*graph, 4096)}
    ms_p = {name: [] for name in kernels}
    for _ in range(a.repeats):
        for name, fn in kernels.items():
            ms_p[name].append(loop_ms(fn))
    molecules = (graph[0] > 0)
    distinct = lambda k: int(torch.unique(k[k != 0]).numel())   # noqa: E731

    # (s) at the shapes of tools/bench_screen.py
    with contextlib.redirect_stdout(sys.stderr):
        inv, fwd = make_synth_model("cfg1", device), make_synth_model("cfg3", device)
    N, K = a.candidates, a.keep
    G = a.screen_rows // N
    cond = synth_normal("bench/screen/cond", (G, 12)).to(device)
    tokens = inv.sample_tokens(cond.repeat(N, 1), device, cond_scale=1.0, timesteps=2, noise=NoiseSource(seed=5))
    wide = SmilesVocabulary({i: ch for i, ch in enumerate("CNOF()=#12cno[]+-", start=1)})      # (some reading of the sampled ids)
    chain = dict(forward_timesteps=a.forward_timesteps, X_norm_factor=16.0, vocabulary=wide, identity="graph")
    screens = {"plain": dict(), "normalize": dict(normalize=True)}

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
    between = med(ms_s["normalize"]) - med(ms_s["plain"])

    result = {"metric": "normal form of the molecular graph", "rows": a.rows, "length": a.length, "repeats": a.repeats,
              "warmup": a.warmup, "rows_that_are_molecules_share": float(molecules.float().mean()),
              "rows_of_status_0_share": float((status == 0).float().mean()),
              "rows_normalised_share": float(((flags & rt.MOLN_NORMALIZED) != 0).float().mean()),
              "rows_with_an_aromatic_ring_share_flag_2": float(((flags & rt.MOLN_AROMATIC) != 0).float().mean()),
              "rows_changed_share_flag_4": float(((flags & rt.MOLN_CHANGED) != 0).float().mean()),
              "distinct_keys_as_written": distinct(keys), "distinct_keys_of_normal_forms": distinct(normal_keys),
              "searches_a_molecule_row_on_the_sample": searches_a_molecule, "ballots_a_molecule_row_on_the_sample": ballots_a_molecule,
              "estimate_rows": len(sample),
              "public_ms": {k: med(v) for k, v in ms_c.items()}, "public_spread_ms": {k: spread(v) for k, v in ms_c.items()},
              "op_ms": {k: med(v) for k, v in ms_p.items()}, "op_spread_ms": {k: spread(v) for k, v in ms_p.items()},
              "mol_normalize_op_over_mol_rings_op": med(ms_p["mol_normalize"]) / med(ms_p["mol_rings"]),
              "mol_normalize_op_estimate_ms": estimate, "mol_normalize_op_measured_over_estimate": med(ms_p["mol_normalize"]) / estimate,
              "screen_rows": a.screen_rows, "screen_tokens_ms": {k: med(v) for k, v in ms_s.items()},
              "screen_tokens_spread_ms": {k: spread(v) for k, v in ms_s.items()}, "normalize_minus_plain_ms": between,
              "difference_inside_the_spread_of_the_two": abs(between) <= max(spread(ms_s["plain"]), spread(ms_s["normalize"])),
              "device": torch.cuda.get_device_name(device)}
    print(json.dumps(result), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
