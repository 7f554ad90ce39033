#!/usr/bin/env python3
"""Writes the rows that tools/molnorm_host_check.cpp checks: the graphs of the reference strings (tests/molkey_ref.py,
tests/smiles_ref.py) with the hydrogens, Kekule structure and verdict of tests/molh_ref.py and the ring sizes of
tests/molring_ref.py, graph arrays that no scan writes, and for each the answer of tests/molnorm_ref.py.

    python tools/molnorm_host_rows.py rows.txt

Lines: "T L n nb atoms_present bonds_present verdict <atoms> <bond words> <atoms_present hydrogens> <atoms_present partner>
<bonds_present bond_ring>" (row t, numbered as they come), "A t flags <L atom words> <L bond words>": the answer for row t."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import molkey_ref as K  # noqa: E402
import molnorm_ref as N  # noqa: E402
import smiles_ref as S  # noqa: E402


def main(path):
    rows = []

    def add(width, s):
        _, _, atoms, bonds = K.graph(s)
        rows.append(N.arrays_row(width, len(atoms), atoms, len(bonds), bonds))
    for s in N.TABLE:
        add(64, s)
        add(max(1, len(s)), s)                                               # as narrow as the string
    for a, b in N.PAIRS:
        add(64, a), add(64, b)
    for g, sp in K.random_spellings():
        for s in sp:
            add(64, s)
    for s in S.mutated_rows(512) + [s for s, _ in S.MALFORMED_TABLE + S.OVERVALENT_TABLE]:
        add(64, s[:64])
    for s in ("C" * 64, "c" * 64, "c1ccccc1" * 8, "*" * 64, "", "C(", "C1C2C3C4C5C6C7C8C9C%10C%11C%12C%13C%14C%15C1C2C3",
              "C12C3C4C1C5C2C3C45", "c1cc2ccc3cccc4ccc(c1)c2c34"):
        add(64, s)
    rows += [row for row, _ in N.special_rows()]
    with open(path, "w") as out:
        for width, n, nb, atoms, bonds, hydrogens, partner, verdict, bond_ring in rows:
            assert len(hydrogens) == len(partner) == len(atoms) and len(bond_ring) == len(bonds)
            out.write("T %d %d %d %d %d %d %s\n" % (width, n, nb, len(atoms), len(bonds), verdict, " ".join(map(
                str, list(atoms) + [N.pack(b) for b in bonds] + list(hydrogens) + list(partner) + list(bond_ring)))))
        for t, row in enumerate(rows):
            r = N.special_answer(row)
            out.write("A %d %d %s\n" % (t, r["flags"], " ".join(map(str, r["atoms"] + r["bonds"]))))


if __name__ == "__main__":
    main(sys.argv[1])
