#!/usr/bin/env python3
"""Writes the rows that tools/molh_host_check.cpp checks: the graphs of the reference strings (tests/molkey_ref.py,
tests/smiles_ref.py), graph arrays that no scan writes, and for each the answer of tests/molh_ref.py with its step count.

    python tools/molh_host_rows.py rows.txt

Lines: "T L n nb atoms_present bonds_present <atoms> <bond words>" (row t, numbered as they come), "H t max_steps verdict atom steps
<L hydrogens> <L partners> <13 formula words>"."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import molh_ref as H  # noqa: E402
import molkey_ref as K  # noqa: E402
import smiles_ref as S  # noqa: E402

RING_MAX = "*" + "0123456789" + ("*" + "0123456789" * 2) * 2 + "*" + "0123456789"
AROMATIC_64 = "c%10ccc(cc%10)c%11ccc(cc%11)c%12ccc(cc%12)c%13ccc(cc%13)c1ccccc1"      # 64 tokens, five rings in a row
TABLE = ["CCO", "CC(=O)O", "CS(C)(=O)=O", "CS(C)=O", "C[N+](=O)[O-]", "[NH4+]", "N#N", "FC(F)(F)F", "ClCCl", "*C", "c1ccccc1", "c1ccncc1",
         "c1cc[nH]c1", "c1ccoc1", "c1ccsc1", "c1cnc[nH]1", "c1ccc2ccccc2c1", "c1ccc2[nH]ccc2c1", "O=c1cccc[nH]1",
         "Cn1cnc2c1c(=O)n(C)c(=O)n2C", "c1ccc2cccc2cc1", "C[n+]1ccccc1", "c1cc[o+]cc1", "[cH-]1cccc1", "Cn1cccc1", "c1ccn2cccc2c1",
         "c1ccccc1-c1ccccc1", "c1ccccc1c1ccccc1", "c1cccc1", "n1cccc1", "c1ccnc1", "c", "cC", "c1ccccc1-c", "c1cc(C)(C)(C)cc1",
         "o1(C)cccc1", "[2H]O[2H]", "c1cc[nH+]cc1", "c1cc[s+]cc1", "[n-]1cccc1", "p1ccccc1", "b1ccccc1", "s1(=O)cccc1", "c1ccs(C)c1",
         "BrCI", "CP(C)(C)=O", "cc", "c:c", "c-c", "c=c", "[se]1cccc1", "[Si](C)(C)C"]


def word(bond):
    a, b, o = bond
    return a | b << 8 | o << 16


def main(path):
    rows, asks = [], []                                                      # (width, n, nb, atoms, bonds (a, b, order)); (t, cap)

    def add(width, s):
        _, _, atoms, bonds = K.graph(s)
        rows.append((width, len(atoms), len(bonds), atoms, bonds))
        asks.append((len(rows) - 1, H.MAX_STEPS))
        return len(rows) - 1
    for s in TABLE:
        add(64, s)
        add(max(1, len(s)), s)                                               # as narrow as the string
    for g, sp in K.random_spellings():
        for s in sp:
            add(64, s)
    for s in S.mutated_rows(512) + [s for s, _ in S.MALFORMED_TABLE + S.OVERVALENT_TABLE]:
        add(64, s[:64])
    for s in ("C" * 64, "c" * 64, RING_MAX, RING_MAX.replace("*", "c"), "c1ccccc1" * 8, "*" * 64, "", "C(", AROMATIC_64,
              "C1C2C3C4C5C6C7C8C9C%10C%11C%12C%13C%14C%15C1C2C3".replace("C", "c")):
        add(64, s)
    for s in ("c1ccc2ccccc2c1", "c1ccc2cccc2cc1", "c1ccccc1", "c" * 64):      # the cap, low
        t = add(64, s)
        asks += [(t, cap) for cap in (1, 2, 3, 31, 32)]
    # arrays that no scan writes: counts outside [0, width], a bond naming a missing atom, an order outside 1..5, a bond listed
    # twice, a bond of an atom to itself, aromatic atoms of symbols the scan never writes in lower case
    c, ar, f = K.descriptor("C"), K.descriptor("c"), K.descriptor("F") | 1 << 10
    for row in [(8, 3, 2, [c] * 3, [(0, 3, 1), (1, 2, 1)]), (8, 9, 0, [], []), (8, 2, 9, [c] * 2, []), (8, -1, 0, [], []),
                (8, 2, -1, [c] * 2, []), (8, 0, 0, [], []), (8, 2, 2, [c] * 2, [(0, 1, 1)] * 2), (8, 2, 1, [c] * 2, [(0, 0, 2)]),
                (8, 2, 1, [c] * 2, [(0, 1, 7)]), (8, 2, 1, [c] * 2, [(0, 1, 0)]), (8, 2, 1, [c] * 2, [(0, 1, 65535)]),
                (8, 2, 2, [ar] * 2, [(0, 1, 5)] * 2), (8, 2, 2, [ar] * 2, [(0, 0, 5), (0, 1, 5)]), (8, 3, 2, [ar] * 3, [(0, 1, 5), (2, 1, 5)]),
                (8, 2, 1, [ar, f], [(0, 1, 5)]), (8, 4, 3, [ar] * 4, [(0, 1, 5), (0, 2, 5), (0, 3, 5)]),
                (8, 8, 8, [ar] * 8, [(i, (i + 1) % 8, 5) for i in range(8)]), (1, 1, 0, [ar], []), (1, 1, 1, [ar], [(0, 0, 5)]),
                (8, 6, 7, [ar] * 6, [(0, 1, 5), (0, 2, 5), (1, 2, 5), (1, 3, 5), (3, 4, 5), (3, 5, 5), (4, 5, 5)])]:      # a try is taken back
        rows.append(row)
        asks.append((len(rows) - 1, H.MAX_STEPS))
    with open(path, "w") as out:
        for width, n, nb, atoms, bonds in rows:
            out.write("T %d %d %d %d %d %s\n" % (width, n, nb, len(atoms), len(bonds), " ".join(map(str, list(atoms) + [word(b) for b in bonds]))))
        for t, cap in asks:
            width, n, nb, atoms, bonds = rows[t]
            r = H.hydrogens_arrays(n, list(atoms), nb, list(bonds), width, cap)
            out.write("H %d %d %d %d %d %s\n" % (t, cap, r["verdict"], r["atom"], r["steps"],
                                                " ".join(map(str, r["hydrogens"] + r["partner"] + r["formula"]))))


if __name__ == "__main__":
    main(sys.argv[1])
