#!/usr/bin/env python3
"""What it costs to ask "which atoms match, and how often?" instead of "does it match?", on the GPU, inputs resident, on the rows of
tools/bench_substructure.py (R = 131072 rows of L = 32 positions, mutated rows of which about half are molecules):

  (p) mdt::sub_map alone                beside mdt::sub_match in the same run, on the graph arrays of those rows, with 1 pattern
                                        (C=O) and the 8 everyday patterns; op calls in a device-event interval, interleaved.
                                        mdt::sub_match is the yardstick: enumeration over first success is the ratio to record.
  (c) substructure_map()                beside has_substructure(), 8 patterns: compaction, mdt::mol_graph, the op, the spread into
                                        bool (R, P, L)
  (k) substructure_keep()               beside scaffold_keep(), 8 patterns
  (s) screen_tokens_diverse(vocabulary=) with and without counts= at 1024 rows (forward cfg3, G = 128, N = 8, K = 2), interleaved
  (u) the share of (row, pattern) pairs with a capped root, and the mean embeddings of a matching pair

    python tools/bench_molmap.py [--rows 131072] [--length 32] [--repeats 9] [--warmup 2]      -> one JSON line

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
from bench_substructure import CLOCK, CYCLES_PER_INSTR, EVERYDAY, INSTR_PER_PATTERN_ATOM, INSTR_PER_ROW, SIMDS  # noqa: E402

# The estimate written down before the first run, from instruction issue as bench_substructure.py's: a pass of
# the enumeration loop is the search's 40 wave instructions and 4 more (the count, the 64-bit OR into the cover, the mask above the
# candidate just taken); a root runs to the end of its tree, so every step is also taken back: 2 * steps + 1 passes (a capped root:
# at most 2 * steps); a pair costs the passes of its slowest root, then the walk of the lowest found root once more up to its first
# success (40 a pass), then 40 instructions to reduce and write the five outputs.
INSTR_PER_ENUM_PASS, INSTR_PER_SEARCH_PASS, INSTR_PER_PAIR = 44, 40, 40


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
    ap.add_argument("--estimate-rows", type=int, default=1024, help="rows whose passes the reference counts for the estimate")
    return ap.parse_args()


def estimate_ms(strings, patterns, rows):
    """The paper estimate of mdt::sub_map from the reference's step counts on a sample of the rows."""
    import molmap_ref as A
    import molsub_ref as B
    instr = 0.0
    for t in strings:
        (ta, tb) = B.graph_of(t)
        instr += INSTR_PER_ROW
        for p in patterns:
            (pa, pb) = B.graph_of(p)
            args = (len(ta), ta, len(tb), tb, len(pa), pa, len(pb), pb)
            if ta and len(pa) <= len(ta):
                instr += INSTR_PER_PATTERN_ATOM * len(pa)
            w = A.map_arrays(*args)
            instr += INSTR_PER_PAIR + INSTR_PER_ENUM_PASS * max([2 * steps + (not cut) for _, _, cut, steps in w["roots"]], default=0)
            if w["found"] and w["roots"]:
                lowest = (w["found"] & -w["found"]).bit_length() - 1
                instr += INSTR_PER_SEARCH_PASS * [s for r, _, s in B.match_arrays(*args)[1] if r == lowest][0]
    return 1e3 * (instr / len(strings)) * CYCLES_PER_INSTR * rows / (SIMDS * CLOCK)


def main():
    a = parse()
    import torch
    from moleculediffusiontransformer_amd import (NoiseSource, SmilesVocabulary, SubstructureCounts, SubstructureSet, has_substructure,
                                                  scaffold_keep, screen_tokens_diverse, substructure_keep, substructure_map)
    from moleculediffusiontransformer_amd import ops  # noqa: F401
    from moleculediffusiontransformer_amd.synth import make_synth_model, synth_normal
    strings = mutated_rows(a.rows, width=a.length)
    vocabulary = SmilesVocabulary([None] + sorted(set("".join(BASES) + ALPHABET + "".join(EVERYDAY))))
    ids = vocabulary.encode(strings, a.length)
    if not torch.cuda.is_available():
        raise SystemExit("bench_molmap.py needs an MI355X: the kernels have no CPU fallback")
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

    def interleaved(legs, measure):
        """warm-up, then ``repeats`` rounds of one measurement per leg -> ({leg: [ms]}, {leg: its last result})"""
        for _ in range(max(1, a.warmup)):
            for leg in legs.values():
                measure(leg)
        ms, last = {name: [] for name in legs}, {}
        for _ in range(a.repeats):
            for name, leg in legs.items():
                got = measure(leg)
                t, last[name] = got if isinstance(got, tuple) else (got, None)
                ms[name].append(t)
        return ms, last

    spread = lambda v: max(v) - min(v)   # noqa: E731
    med = statistics.median
    report = lambda ms: ({k: med(v) for k, v in ms.items()}, {k: spread(v) for k, v in ms.items()})  # noqa: E731

    # (p): the two ops alone, interleaved
    packed, length, _, _ = torch.ops.mdt.tokens_compact(tok.int(), 0, 1.0)
    graph = torch.ops.mdt.mol_graph(packed, length, *tables)[:4]
    ops_p = {}
    for P in sets:
        ops_p[f"sub_match_{P}"] = lambda P=P: torch.ops.mdt.sub_match(*graph, *sets[P].on(device), 0, 0)
        ops_p[f"sub_map_{P}"] = lambda P=P: torch.ops.mdt.sub_map(*graph, *sets[P].on(device), None, None)
    ms_p, _ = interleaved(ops_p, loop_ms)
    sample = strings[:: max(1, a.rows // a.estimate_rows)]
    estimate = {P: estimate_ms(sample, list(sets[P].patterns), a.rows) for P in sets}

    # (c), (k): the public calls, interleaved
    public = {"has_substructure_8": lambda: has_substructure(tok, sets[8], vocabulary, device),
              "substructure_map_8": lambda: substructure_map(tok, sets[8], vocabulary, device),
              "scaffold_keep": lambda: scaffold_keep(tok, vocabulary, device),
              "substructure_keep_8": lambda: substructure_keep(tok, sets[8], vocabulary, device)}
    ms_c, last = interleaved(public, once)
    mapped = last["substructure_map_8"]
    matching = mapped.count > 0

    # (s) at the shapes of tools/bench_screen.py
    with contextlib.redirect_stdout(sys.stderr):
        inv, fwd = make_synth_model("cfg1", device), make_synth_model("cfg3", device)
    N, K = a.candidates, a.keep
    G = a.screen_rows // N
    cond = synth_normal("bench/screen/cond", (G, 12)).to(device)
    tokens = inv.sample_tokens(cond.repeat(N, 1), device, cond_scale=1.0, timesteps=2, noise=NoiseSource(seed=5))
    wide = SmilesVocabulary({i: ch for i, ch in enumerate("CNOF()=#12cno[]+-", start=1)})      # (some reading of the sampled ids)
    chain = dict(forward_timesteps=a.forward_timesteps, X_norm_factor=16.0, vocabulary=wide)
    few = SubstructureCounts(["[N+](=O)[O-]", "n", "F"], wide, at_least=[None, None, None], at_most=[1, 2, 3])
    few.set.on(device), few.on(device)
    screens = {"plain": dict(), "counts": dict(counts=few)}
    seeds = iter(range(900, 10 ** 6))
    legs_s = {leg: (lambda kw=kw: screen_tokens_diverse(fwd, tokens, cond, device, N, K, forward_noise=NoiseSource(seed=next(seeds)),
                                                        **kw, **chain)) for leg, kw in screens.items()}
    ms_s, _ = interleaved(legs_s, once)
    between = med(ms_s["counts"]) - med(ms_s["plain"])

    op_ms, op_spread = report(ms_p)
    public_ms, public_spread = report(ms_c)
    screen_ms, screen_spread = report(ms_s)
    result = {"metric": "graph substructure enumeration", "rows": a.rows, "length": a.length, "repeats": a.repeats, "warmup": a.warmup,
              "patterns": EVERYDAY, "pairs_matched_share": float(matching.float().mean()),
              "pairs_with_a_capped_root_share": float(mapped.undecided.float().mean()),
              "mean_embeddings_of_a_matching_pair": float(mapped.embeddings[matching].float().mean()),
              "mean_anchors_of_a_matching_pair": float(mapped.count[matching].float().mean()),
              "op_ms": op_ms, "op_spread_ms": op_spread,
              "sub_map_over_sub_match": {str(P): op_ms[f"sub_map_{P}"] / op_ms[f"sub_match_{P}"] for P in sets},
              "sub_map_op_estimate_ms": {str(P): estimate[P] for P in sets}, "estimate_rows": len(sample),
              "sub_map_op_measured_over_estimate": {str(P): op_ms[f"sub_map_{P}"] / estimate[P] for P in sets},
              "public_ms": public_ms, "public_spread_ms": public_spread,
              "screen_rows": a.screen_rows, "screen_tokens_ms": screen_ms, "screen_tokens_spread_ms": screen_spread,
              "counts_minus_plain_ms": between, "difference_inside_the_spread_of_plain": abs(between) <= spread(ms_s["plain"]),
              "device": torch.cuda.get_device_name(device)}
    print(json.dumps(result), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
