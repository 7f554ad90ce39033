#!/usr/bin/env python3
"""What it costs to ask "what do these two molecules share?", on the GPU, inputs resident, on the rows of the other bench_mol*.py
(R = 131072 rows of L = 32 positions, mutated rows of which about half are molecules), in two pairings:

  next     row r against row r + 1 (two unrelated rows; a pair is a pair of molecules in about a quarter of the cases)
  edited   every row against a copy with one or two random token substitutions that is still a molecule where the row is one (up to
           four tries a row, else the row itself): the generated-versus-target case

  (p) mdt::mol_mcs alone                beside mdt::sub_map with one pattern (C=O) and beside mdt::mol_canon on the same rows -- the
                                        two yardsticks: the nearest search kernels -- op calls in a device-event interval, interleaved
  (c) mol_mcs() as a call               compaction and mdt::mol_graph for both sides, the op, the masks and the similarity
  (u) steps a pair (mean, maximum), the undecided share, the shares of the flags

    python tools/bench_molmcs.py [--rows 131072] [--length 32] [--repeats 9] [--warmup 2]      -> one JSON line

Reported: medians and spreads (max - min) in ms, and the paper estimate of (p) beside its measurement.  There is no pass mark.
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
from bench_substructure import CLOCK, CYCLES_PER_INSTR, EVERYDAY, SIMDS  # noqa: E402

# The estimate written down before the first run: instruction issue, not latency, as bench_substructure.py's.  One wave a pair; its
# lanes take the na * nb roots in rounds of 64, and a round costs what its slowest lane costs.  A pass of the walk's loop -- the
# bound over five orders, the pick over the frontier entries, an assignment or its undoing with the count computed again -- is
# about 150 wave instructions; a root of s steps makes s passes forward and about as many back: 2 s + 1.  A greedy descent is a pick
# and an assignment a mapped atom, about 90.  Per pair 450 instructions to check, stage and build both sides' tables and to write
# the ten outputs, 14 per A atom for the compat ballot and the prefix OR; then the winner's walk once more up to its best (at most
# its own passes; counted in full).  A pair that is no pair costs the check and the zeros, 60.  1024 SIMDs at 2.4 GHz.
INSTR_PER_PASS, INSTR_PER_GREEDY_ATOM, INSTR_PER_PAIR, INSTR_PER_A_ATOM, INSTR_NO_PAIR = 150, 90, 450, 14, 60


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=131072)
    ap.add_argument("--length", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel-loop", type=int, default=10, help="op calls per device-event interval of (p)")
    ap.add_argument("--estimate-rows", type=int, default=512, help="pairs whose passes the reference counts for the estimate")
    return ap.parse_args()


def estimate_ms(pairs, rows):
    """The paper estimate of mdt::mol_mcs from the reference's step counts on a sample of the pairs."""
    import molmcs_ref as C
    sys.setrecursionlimit(10000)
    instr = 0.0
    for a, b in pairs:
        w = C.string_mcs(a, b)
        if not w["flags"]:
            instr += INSTR_NO_PAIR
            continue
        na, nb = len(C.graph_of(a)[0]), len(C.graph_of(b)[0])
        instr += INSTR_PER_PAIR + INSTR_PER_A_ATOM * na
        by_round = {}
        for a0, b0, _, atoms, steps, _ in w["roots"]:
            k = (a0 * nb + b0) // 64
            by_round[k] = max(by_round.get(k, 0), steps)
        instr += sum(INSTR_PER_PASS * (2 * s + 1) + INSTR_PER_GREEDY_ATOM * min(na, nb) for s in by_round.values())
        instr += INSTR_PER_PASS * max([r[4] for r in w["roots"]], default=0)
    return 1e3 * (instr / max(1, len(pairs))) * CYCLES_PER_INSTR * rows / (SIMDS * CLOCK)


def main():
    a = parse()
    import numpy as np
    import torch
    from moleculediffusiontransformer_amd import SmilesVocabulary, SubstructureSet, mol_mcs, runtime as rt, smiles_check
    from moleculediffusiontransformer_amd import ops  # noqa: F401
    strings = mutated_rows(a.rows, width=a.length)
    vocabulary = SmilesVocabulary([None] + sorted(set("".join(BASES) + ALPHABET + "".join(EVERYDAY))))
    ids = vocabulary.encode(strings, a.length)
    if not torch.cuda.is_available():
        raise SystemExit("bench_molmcs.py needs an MI355X: the kernels have no CPU fallback")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    tok = ids.to(device)
    tables = vocabulary.on(device)
    one = SubstructureSet(EVERYDAY[:1], vocabulary)
    one.on(device)

    # the edited copies: up to four tries a row, the first that is still a molecule
    rng = np.random.default_rng(23)
    base = ids.numpy()
    length = (base != 0).sum(1)
    ok = smiles_check(tok, vocabulary, device)[0].cpu().numpy() == 0
    edited = base.copy()
    settled = ~ok | (length == 0)
    for _ in range(4):
        cand = base.copy()
        for edit in range(2):
            hit = rng.random(a.rows) < (1.0 if edit == 0 else 0.5)
            pos = (rng.random(a.rows) * np.maximum(length, 1)).astype(np.int64)
            new = rng.integers(1, len(vocabulary) + 1, a.rows)
            rows_hit = np.nonzero(hit)[0]
            cand[rows_hit, pos[rows_hit]] = new[rows_hit]
        good = smiles_check(torch.from_numpy(cand).to(device), vocabulary, device)[0].cpu().numpy() == 0
        take = ~settled & good & (cand != base).any(1)
        edited[take] = cand[take]
        settled |= take
    pairings = {"next": torch.roll(tok, -1, 0), "edited": torch.from_numpy(edited).to(device)}
    other_strings = {"next": strings[1:] + strings[:1], "edited": vocabulary.decode(torch.from_numpy(edited))}

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

    def graph_of(t):
        packed, n, _, _ = torch.ops.mdt.tokens_compact(t.int(), 0, 1.0)
        return torch.ops.mdt.mol_graph(packed, n, *tables)[:4]
    graph = graph_of(tok)
    others = {name: graph_of(t) for name, t in pairings.items()}
    ops_p = {"sub_map_1": lambda: torch.ops.mdt.sub_map(*graph, *one.on(device), None, None),
             "mol_canon": lambda: torch.ops.mdt.mol_canon(*graph)}
    for name in pairings:
        ops_p[f"mol_mcs_{name}"] = lambda name=name: torch.ops.mdt.mol_mcs(*graph, *others[name], 0)
    ms_p, _ = interleaved(ops_p, loop_ms)
    step = max(1, a.rows // a.estimate_rows)
    estimate = {name: estimate_ms(list(zip(strings[::step], other_strings[name][::step])), a.rows) for name in pairings}

    public = {f"mol_mcs_{name}": (lambda name=name: mol_mcs(tok, pairings[name], vocabulary, device)) for name in pairings}
    ms_c, last = interleaved(public, once)

    op_ms, op_spread = report(ms_p)
    public_ms, public_spread = report(ms_c)
    result = {"metric": "maximum common substructure of row pairs", "rows": a.rows, "length": a.length, "repeats": a.repeats,
              "warmup": a.warmup, "op_ms": op_ms, "op_spread_ms": op_spread,
              "mol_mcs_over_sub_map_1": {n: op_ms[f"mol_mcs_{n}"] / op_ms["sub_map_1"] for n in pairings},
              "mol_mcs_over_mol_canon": {n: op_ms[f"mol_mcs_{n}"] / op_ms["mol_canon"] for n in pairings},
              "mol_mcs_op_estimate_ms": estimate, "estimate_pairs": len(strings[::step]),
              "mol_mcs_op_measured_over_estimate": {n: op_ms[f"mol_mcs_{n}"] / estimate[n] for n in pairings},
              "public_ms": public_ms, "public_spread_ms": public_spread, "edited_rows_share": float((edited != base).any(1).mean())}
    for name in pairings:
        r = last[f"mol_mcs_{name}"]
        pair = r.pair
        result[name] = {"pairs_share": float(pair.float().mean()), "undecided_share": float(r.undecided.float().mean()),
                        "steps_mean_of_a_pair": float(r.steps[pair].float().mean()) if bool(pair.any()) else 0.0,
                        "steps_max": int(r.steps.max()), "whole_a_share": float(r.whole_a.float().mean()),
                        "mean_atoms_shared": float(r.atoms[pair].float().mean()) if bool(pair.any()) else 0.0,
                        "mean_similarity": float(r.similarity[pair].mean()) if bool(pair.any()) else 0.0}
    result["device"] = torch.cuda.get_device_name(device)
    result["cap"] = rt.MCS_MAX_STEPS
    print(json.dumps(result), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
