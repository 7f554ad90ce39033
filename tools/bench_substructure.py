#!/usr/bin/env python3
"""What it costs to ask "does the molecule contain this fragment?" of generated rows, on the GPU, inputs resident:

  (c) has_substructure()               R = 131072 rows of L = 32 positions, the mutated rows of tools/bench_smiles.py (about half are
                                       molecules, the rest contain nothing), with 1 pattern (C=O) and with the 8 everyday patterns
                                       C=O C#N c1ccccc1 C1CC1 CC(=O)O N [O-] C(F)(F)F: compaction, mdt::mol_graph, mdt::sub_match, the
                                       spread into bool (R, P) -- beside mol_key() and mol_fingerprint() on the same rows
  (p) mdt::sub_match alone             the graph arrays of those rows; op calls in a device-event interval; 1 and 8 patterns
  (u) the share of (row, pattern) pairs that came out undecided, and that matched
  (s) screen_tokens_diverse(vocabulary=) with and without require= / forbid= at 1024 rows (forward cfg3, G = 128, N = 8, K = 2),
      interleaved

    python tools/bench_substructure.py [--rows 131072] [--length 32] [--repeats 9] [--warmup 2]      -> one JSON line

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

EVERYDAY = ["C=O", "C#N", "c1ccccc1", "C1CC1", "CC(=O)O", "N", "[O-]", "C(F)(F)F"]
# The estimate written down before the first run: instruction issue, not latency (enough waves are resident to hide the LDS round
# trips).  A wave's roots search side by side, so a (row, pattern) pair costs the passes of its slowest root; a pass of the search
# loop is about 40 wave instructions (the back-bonds, the map, 64-bit masks), i.e. 160 cycles a step on a SIMD that takes 4 cycles
# per wave instruction; per row 250 instructions to check, stage and build the adjacency and to write out, per pattern atom 12 for
# the ballot.  1024 SIMDs at 2.4 GHz; memory traffic (34 MB of graph arrays) is below that.
INSTR_PER_PASS, INSTR_PER_ROW, INSTR_PER_PATTERN_ATOM = 40, 250, 12
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
    ap.add_argument("--estimate-rows", type=int, default=1024, help="rows whose search passes the reference counts for the estimate")
    return ap.parse_args()


def estimate_ms(strings, patterns, rows):
    """The paper estimate of mdt::sub_match from the reference's step counts on a sample of the rows."""
    import molsub_ref as B
    cycles = 0.0                                                             # (wave instructions, until the last line)
    for t in strings:
        (ta, tb) = B.graph_of(t)
        cycles += INSTR_PER_ROW
        for p in patterns:
            (pa, pb) = B.graph_of(p)
            verdict, roots = B.match_arrays(len(ta), ta, len(tb), tb, len(pa), pa, len(pb), pb)
            if ta and len(pa) <= len(ta):
                cycles += INSTR_PER_PATTERN_ATOM * len(pa)
            # a root that fails takes every step back as well: two passes a step
            cycles += INSTR_PER_PASS * max([s if v == B.MATCH else 2 * s + 1 for _, v, s in roots], default=0)
    return 1e3 * (cycles / len(strings)) * CYCLES_PER_INSTR * rows / (SIMDS * CLOCK)


def main():
    a = parse()
    import torch
    from moleculediffusiontransformer_amd import (NoiseSource, SmilesVocabulary, SubstructureSet, has_substructure, mol_fingerprint,
                                                  mol_key, screen_tokens_diverse)
    from moleculediffusiontransformer_amd import ops  # noqa: F401
    from moleculediffusiontransformer_amd.synth import make_synth_model, synth_normal
    strings = mutated_rows(a.rows, width=a.length)
    vocabulary = SmilesVocabulary([None] + sorted(set("".join(BASES) + ALPHABET + "".join(EVERYDAY))))
    ids = vocabulary.encode(strings, a.length)
    if not torch.cuda.is_available():
        raise SystemExit("bench_substructure.py needs an MI355X: the kernels have no CPU fallback")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    tok = ids.to(device)
    tables = vocabulary.on(device)
    sets = {1: SubstructureSet(EVERYDAY[:1], vocabulary), 8: SubstructureSet(EVERYDAY, vocabulary)}
    for one in sets.values():
        one.on(device)

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
    legs = {"has_substructure_1": lambda: has_substructure(tok, sets[1], vocabulary, device),
            "has_substructure_8": lambda: has_substructure(tok, sets[8], vocabulary, device),
            "mol_key": lambda: mol_key(tok, vocabulary, device),
            "mol_fingerprint": lambda: mol_fingerprint(tok, vocabulary, device, a.radius)}
    for _ in range(a.warmup):
        for leg in legs.values():
            once(leg)
    ms_c = {name: [] for name in legs}
    for _ in range(a.repeats):
        for name, leg in legs.items():
            t, out = once(leg)
            ms_c[name].append(t)
            if name == "has_substructure_8":
                match, undecided = out[0], out[1]
    # (p): the op alone
    packed, length, _, _ = torch.ops.mdt.tokens_compact(tok.int(), 0, 1.0)
    graph = torch.ops.mdt.mol_graph(packed, length, *tables)[:4]
    ms_p = {P: [loop_ms(lambda: torch.ops.mdt.sub_match(*graph, *sets[P].on(device), 0, 0)) for _ in range(a.repeats)] for P in sets}
    sample = strings[:: max(1, a.rows // a.estimate_rows)]
    estimate = {P: estimate_ms(sample, list(sets[P].patterns), a.rows) for P in sets}

    # (s) at the shapes of tools/bench_screen.py
    with contextlib.redirect_stdout(sys.stderr):
        inv, fwd = make_synth_model("cfg1", device), make_synth_model("cfg3", device)
    N, K = a.candidates, a.keep
    G = a.screen_rows // N
    cond = synth_normal("bench/screen/cond", (G, 12)).to(device)
    tokens = inv.sample_tokens(cond.repeat(N, 1), device, cond_scale=1.0, timesteps=2, noise=NoiseSource(seed=5))
    wide = SmilesVocabulary({i: ch for i, ch in enumerate("CNOF()=#12cno[]+-", start=1)})      # (some reading of the sampled ids)
    chain = dict(forward_timesteps=a.forward_timesteps, X_norm_factor=16.0, vocabulary=wide)
    want, never = SubstructureSet(["C=O", "N"], wide), SubstructureSet(["C#N", "OO", "[O-]"], wide)
    want.on(device), never.on(device)
    screens = {"plain": dict(), "fragments": dict(require=want, forbid=never)}

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
    between = med(ms_s["fragments"]) - med(ms_s["plain"])

    result = {"metric": "graph substructure match", "rows": a.rows, "length": a.length, "repeats": a.repeats, "warmup": a.warmup,
              "patterns": EVERYDAY, "pairs_matched_share": float(match.float().mean()),
              "pairs_undecided_share": float(undecided.float().mean()), "rows_with_a_match": int(match.any(dim=1).sum()),
              "public_ms": {k: med(v) for k, v in ms_c.items()}, "public_spread_ms": {k: spread(v) for k, v in ms_c.items()},
              "sub_match_op_ms": {str(P): med(v) for P, v in ms_p.items()},
              "sub_match_op_spread_ms": {str(P): spread(v) for P, v in ms_p.items()},
              "sub_match_op_estimate_ms": {str(P): estimate[P] for P in sets}, "estimate_rows": len(sample),
              "sub_match_op_measured_over_estimate": {str(P): med(ms_p[P]) / estimate[P] for P in sets},
              "screen_rows": a.screen_rows, "screen_tokens_ms": {k: med(v) for k, v in ms_s.items()},
              "screen_tokens_spread_ms": {k: spread(v) for k, v in ms_s.items()}, "fragments_minus_plain_ms": between,
              "difference_inside_the_spread_of_plain": abs(between) <= spread(ms_s["plain"]),
              "device": torch.cuda.get_device_name(device)}
    print(json.dumps(result), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
