#!/usr/bin/env python3
"""Writes the rows that tools/molscaf_host_check.cpp checks: the graphs of the reference strings (tests/molkey_ref.py,
tests/smiles_ref.py) as written and as normal forms (tests/molnorm_ref.py), graph arrays that no scan writes, and for each, in each
of the four modes, the answer of tests/molscaf_ref.py.

    python tools/molscaf_host_rows.py rows.txt

Lines: "T L n nb atoms_present bonds_present <atoms> <bond words>" (row t, numbered as they come), "A t mode natoms nbonds flags
<L atom words> <L bond words> <L atom_map bytes>": the answer for row t in that mode."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import molkey_ref as K  # noqa: E402
import molnorm_ref as N  # noqa: E402
import molscaf_ref as C  # noqa: E402
import smiles_ref as S  # noqa: E402


def main(path):
    rows = []

    def add(width, s, normalize=False):
        n, atoms, nb, bonds = C.input_arrays(s, normalize, width)
        rows.append((width, n, nb, atoms, bonds))
    for s in list(C.TABLE) + list(N.TABLE):
        add(64, s), add(64, s, True)
        add(max(1, len(s)), s)                                               # as narrow as the string
    for g, sp in K.random_spellings():
        for s in sp:
            add(64, s)
        add(64, sp[0], True)
    for s in S.mutated_rows(512) + [s for s, _ in S.MALFORMED_TABLE + S.OVERVALENT_TABLE]:
        add(64, s[:64])
    for s in ("C" * 64, "c" * 64, "c1ccccc1" * 8, "*" * 64, "", "C(", "C1CC1" + "C" * 59, "C1" + "C" * 60 + "C1", "C1CC1" + "C" * 54 + "C1CC1",
              "C12C3C4C1C5C2C3C45", "c1cc2ccc3cccc4ccc(c1)c2c34", "O=C1C(=O)C(=O)C1=O"):
        add(64, s)
    rows += C.special_rows()
    with open(path, "w") as out:
        for width, n, nb, atoms, bonds in rows:
            out.write("T %d %d %d %d %d %s\n" % (width, n, nb, len(atoms), len(bonds), " ".join(map(str, list(atoms) + [N.pack(b) for b in bonds]))))
        for t, (width, n, nb, atoms, bonds) in enumerate(rows):
            for mode in C.MODES:
                r = C.scaffold_arrays(n, atoms, nb, bonds, mode, width)
                out.write("A %d %d %d %d %d %s\n" % (t, mode, r["n"], r["nb"], r["flags"], " ".join(map(str, r["atoms"] + r["bonds"] + r["atom_map"]))))


if __name__ == "__main__":
    main(sys.argv[1])
