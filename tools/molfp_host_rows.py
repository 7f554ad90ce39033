#!/usr/bin/env python3
"""Writes the rows that tools/molfp_host_check.cpp checks: the graphs of the reference strings (tests/molkey_ref.py,
tests/smiles_ref.py) with their expected fingerprints from tests/molfp_ref.py, pairs with their expected counts and threshold
verdicts, and nearest searches with their expected winners.

    python tools/molfp_host_rows.py rows.txt

Lines: "R L n nb radius atoms_present bonds_present <atoms> <bonds> <16 hex words> count", "P a b inter union sim_num at_least",
"N q m index inter union" (query row q against rows 0 .. m - 1)."""
import os
import random
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import molfp_ref as F  # noqa: E402
import molkey_ref as K  # noqa: E402
import smiles_ref as S  # noqa: E402


def main(path):
    rng = random.Random(3)
    strings = [s for pair in K.EQUAL_PAIRS + K.DIFFERENT_PAIRS for s in pair] + [s for s, _, _ in S.TABLES] + ["", "C" * 64]
    strings += [s for _, sp in K.random_spellings() for s in sp] + S.mutated_rows()
    rows = []                                                                # (L, n, nb, radius, atoms, bond words)
    for i, s in enumerate(strings):
        _, _, atoms, bonds = K.graph(s)
        rows.append((64, len(atoms), len(bonds), i % 4 if i % 7 else 2, atoms, [a | b << 8 | o << 16 for a, b, o in bonds]))
    c = K.descriptor("C")
    rows += [(8, 3, 2, 2, [c] * 3, [0 | 3 << 8 | 1 << 16, 1 | 2 << 8 | 1 << 16]),      # a bond names atom 3 of 3: no molecule
             (8, 9, 0, 2, [], []), (8, 2, 9, 2, [c] * 2, []), (8, -1, 0, 2, [], []), (8, 2, -1, 2, [c] * 2, []),
             (8, 2, 2, 3, [c] * 2, [0 | 1 << 8 | 1 << 16] * 2),                       # a bond listed twice counts twice
             (8, 2, 1, 3, [c] * 2, [0 | 0 << 8 | 2 << 16])]                           # a bond of an atom to itself
    fps = []
    with open(path, "w") as f:
        for L, n, nb, radius, atoms, bonds in rows:
            ok = 1 <= n <= L and 0 <= nb <= L
            fp = F.fingerprint(atoms, [(w & 255, w >> 8 & 255, w >> 16) for w in bonds], radius, L) if ok else 0
            fps.append(fp)
            f.write("R %d %d %d %d %d %d %s %s %d\n" % (L, n, nb, radius, len(atoms), len(bonds), " ".join(map(str, atoms + bonds)),
                                                        " ".join("%x" % w for w in F.words(fp)), F.popcount(fp)))
        for _ in range(20000):
            a, b = rng.randrange(len(fps)), rng.randrange(len(fps))
            if rng.random() < 0.2:
                b = a
            inter, union = F.counts(fps[a], fps[b])
            sim_num = rng.choice([1, 65536, 32768, rng.randint(1, 65536), max(1, min(65536, inter * 65536 // max(union, 1) + rng.randint(-1, 1)))])
            f.write("P %d %d %d %d %d %d\n" % (a, b, inter, union, sim_num, int(F.at_least(inter, union, sim_num))))
        m = 1000
        for q in list(range(150)) + [len(fps) - k for k in range(1, 8)]:
            f.write("N %d %d %d %d %d\n" % ((q, m) + F.nearest(fps[q], fps[:m])))


if __name__ == "__main__":
    main(sys.argv[1])
