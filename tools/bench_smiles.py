#!/usr/bin/env python3
"""What it costs to ask "is it a molecule at all?" of every generated row, on the GPU, inputs resident:

  (c) smiles_check()                  R = 131072 rows of L = 32 positions drawn by the mutation recipe of tests/smiles_ref.py (seed 11:
                                      OK strings with 0, 1 or 2 random edits -- about half pass, two in five are malformed, one in
                                      thirteen overvalent): compaction and mdt::smiles_check, one host synchronisation per call
  (k) mdt::smiles_check alone         the same rows, compacted once; op calls in a device-event interval
  (p) mdt::tokens_compact alone       the same rows: a pass over the same bytes, the yardstick of (k)
  (s) screen_tokens_diverse(vocabulary=) beside screen_tokens() at 1024 rows (forward cfg3, G = 128, N = 8, K = 2), interleaved

    python tools/bench_smiles.py [--rows 131072] [--length 32] [--repeats 9] [--warmup 2]      -> one JSON line

Reported: medians and spreads (max - min) in ms, rows per second of (k), and (k) over (p).  There is no pass mark.
"""
import argparse
import contextlib
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# the recipe of tests/smiles_ref.py, restated so that the tool stands without the tests
BASES = ("C CC C=C C#N CCO CC(=O)O C1CC1 C1CC1C c1ccccc1 OC1CC1 C1=CC=CC=C1 CC(C)(C)C N#CC#N FC(F)(F)F ClCCl BrCBr C(Cl)Cl [NH4+] "
         "[O-]C=O C[N+](C)(C)C [nH]1cccc1 c1cc[nH]c1 C12CC1C2 C1CC2CC12 C%10CC%10 C%10CC%10C1CC1 C/C=C/C C/C=C\\C F/C=C/F "
         "[C@H](N)(O)C [C@@H](N)(O)C C.C [Na+].[Cl-] C1.C1 CC(C)1CC1 C=1CC1 C1CC=1 C=1CC=1 O=C1CC1 N1C=CC=C1 CS(=O)(=O)C "
         "CP(=O)(O)O C(=O)=O [13CH4] [2H]O[2H] [C:12]C C(C) C(C)(C) C(-C)C C(=O)C *C [*]C C$C CC1=CC(=O)C2CC2C1 OC1C2CC3CC1C3O2 "
         "N#CC1(CC1)C#N CC1OC2CC1C2O O=CC1=CNC=N1 C1C2C3C1C1C2C31 CC12CC1C1OC21 c1cc2cc[nH]c2o1").split()
ALPHABET = "CNOFcno()=#12[]H+-.l%/"


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
    ap.add_argument("--kernel-loop", type=int, default=20, help="op calls per device-event interval of (k) and (p)")
    return ap.parse_args()


def mutated_rows(rows, seed=11, width=32):
    rng = random.Random(seed)
    bases = [s for s in BASES if len(s) <= 28]
    out = []
    for r in range(rows):
        s = list(rng.choice(bases))
        for _ in range(r % 3):
            kind = rng.randrange(4)
            if kind == 0 and s:
                s[rng.randrange(len(s))] = rng.choice(ALPHABET)
            elif kind == 1:
                s.insert(rng.randrange(len(s) + 1), rng.choice(ALPHABET))
            elif kind == 2 and s:
                del s[rng.randrange(len(s))]
            elif kind == 3:
                spots = [i for i, ch in enumerate(s) if ch in "CNOF"]
                if spots:
                    i = rng.choice(spots) + 1
                    s[i:i] = list(rng.choice(["(F)", "(=O)", "(C)(C)"]))
        out.append("".join(s)[:width])
    return out


def main():
    a = parse()
    import torch
    from moleculediffusiontransformer_amd import NoiseSource, SmilesVocabulary, screen_tokens, screen_tokens_diverse, smiles_check
    from moleculediffusiontransformer_amd import ops  # noqa: F401
    from moleculediffusiontransformer_amd.synth import make_synth_model, synth_normal
    strings = mutated_rows(a.rows, width=a.length)
    vocabulary = SmilesVocabulary([None] + sorted(set("".join(BASES) + ALPHABET)))
    ids = vocabulary.encode(strings, a.length)
    mean_length = sum(len(s) for s in strings) / len(strings)
    if not torch.cuda.is_available():
        raise SystemExit("bench_smiles.py needs an MI355X: the check has no CPU fallback")
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

    # (c), (k), (p)
    for _ in range(a.warmup):
        once(lambda: smiles_check(tok, vocabulary, device))
    ms_c = []
    for _ in range(a.repeats):
        t, (status, position) = once(lambda: smiles_check(tok, vocabulary, device))
        ms_c.append(t)
    tok32 = tok.int()
    packed, length, _, _ = torch.ops.mdt.tokens_compact(tok32, 0, 1.0)
    ms_k = [loop_ms(lambda: torch.ops.mdt.smiles_check(packed, length, *tables)) for _ in range(a.repeats)]
    ms_p = [loop_ms(lambda: torch.ops.mdt.tokens_compact(tok32, 0, 1.0)) for _ in range(a.repeats)]
    med_c, med_k, med_p = statistics.median(ms_c), statistics.median(ms_k), statistics.median(ms_p)
    verdicts = {name: int((status == v).sum()) for name, v in (("ok", 0), ("malformed", 32), ("overvalent", 64))}

    # (s) at the shapes of tools/bench_screen.py
    with contextlib.redirect_stdout(sys.stderr):
        inv, fwd = make_synth_model("cfg1", device), make_synth_model("cfg3", device)
    N, K = a.candidates, a.keep
    G = a.screen_rows // N
    cond = synth_normal("bench/screen/cond", (G, 12)).to(device)
    tokens = inv.sample_tokens(cond.repeat(N, 1), device, cond_scale=1.0, timesteps=2, noise=NoiseSource(seed=5))
    wide = SmilesVocabulary({i: ch for i, ch in enumerate("CNOF()=#12cno[]+-", start=1)})      # (some reading of the sampled ids)
    chain = dict(forward_timesteps=a.forward_timesteps, X_norm_factor=16.0)

    def plain(i):
        return screen_tokens(fwd, tokens, cond, device, N, K, forward_noise=NoiseSource(seed=900 + i), **chain)

    def checked(i):
        return screen_tokens_diverse(fwd, tokens, cond, device, N, K, vocabulary=wide, forward_noise=NoiseSource(seed=900 + i), **chain)
    for w in range(max(1, a.warmup)):
        once(lambda: plain(-1 - w))
        once(lambda: checked(-1 - w))
    ms_s = {"plain": [], "vocabulary": []}
    valid = 0.0
    for i in range(a.repeats):                       # interleaved: one of each per repeat
        ms_s["plain"].append(once(lambda: plain(i))[0])
        t, out = once(lambda: checked(i))
        ms_s["vocabulary"].append(t)
        valid = float(((out.status & 96) == 0).float().mean())
    med_s = {k: statistics.median(v) for k, v in ms_s.items()}

    spread = lambda v: max(v) - min(v)   # noqa: E731
    result = {"metric": "well-formedness and valence of token rows", "rows": a.rows, "length": a.length, "mean_row_length": mean_length,
              "repeats": a.repeats, "warmup": a.warmup, "verdicts": verdicts,
              "smiles_check_ms": med_c, "smiles_check_spread_ms": spread(ms_c),
              "smiles_check_op_ms": med_k, "smiles_check_op_spread_ms": spread(ms_k), "rows_per_s": a.rows / (1e-3 * med_k),
              "tokens_compact_op_ms": med_p, "tokens_compact_op_spread_ms": spread(ms_p), "check_over_compact": med_k / med_p,
              "screen_rows": a.screen_rows, "screen_tokens_ms": med_s, "screen_tokens_spread_ms": {k: spread(v) for k, v in ms_s.items()},
              "vocabulary_minus_plain_ms": med_s["vocabulary"] - med_s["plain"], "valid_fraction_last_repeat": valid,
              "device": torch.cuda.get_device_name(device)}
    print(json.dumps(result), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
