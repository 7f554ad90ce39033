#!/usr/bin/env python3
"""Writes the rows that tools/molcanon_host_check.cpp checks: the graphs of the reference strings (tests/molkey_ref.py,
tests/smiles_ref.py) as written and as normal forms (tests/molnorm_ref.py), symmetric molecules under renumbering, rows above the
node cap, graph arrays that no scan writes, and for each the answer of tests/molcanon_ref.py.

    python tools/molcanon_host_rows.py rows.txt

Lines: "T L n nb atoms_present bonds_present <atoms> <bond words>" (row t, numbered as they come), "Q t flags nodes <L priority
words> <L canon_atoms words> <L canon_bonds words>": mdt_mol_canon's answer for row t (nodes: -1 for an undecided row, where any
value above the cap is right)."""
import os
import random
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import molcanon_ref as Q  # noqa: E402
import molkey_ref as K  # noqa: E402
import molnorm_ref as N  # noqa: E402
import molscaf_ref as C  # noqa: E402
import molwrite_ref as W  # noqa: E402
import smiles_ref as S  # noqa: E402

SYMMETRIC = ["C12C3C4C1C5C2C3C45", "C1C2CC3CC1CC(C2)C3", "c1cc2ccc3ccc4ccc5ccc6ccc1c1c2c3c4c5c61", "C12C3C4C1C5C2C3C45.C12C3C4C1C5C2C3C45",
             "C12C3C4C5C1C1C6C2C2C3C3C4C4C5C1C1C6C2C3C41", "CC(C)(C)C", "FC(F)(F)C(F)(F)F", "CC.CC.CC", "[NH4+].[Cl-].[NH4+].[Cl-]",
             "c1ccccc1c1c(c2ccccc2)c(c2ccccc2)c(c2ccccc2)c(c2ccccc2)c1c1ccccc1",
             "c1ccccc1C(c1ccccc1)(c1ccccc1)C(c1ccccc1)(c1ccccc1)c1ccccc1", ".".join(["[Cl-]"] * 8)]


def main(path):
    rows = []

    def add(width, s, normalize=False):
        n, atoms, nb, bonds = C.input_arrays(s, normalize, width)
        rows.append((width, n, nb, atoms, bonds))
    for s in list(C.TABLE) + list(N.TABLE):
        add(64, s), add(64, s, True)
        add(max(1, len(s)), s)                                               # as narrow as the string
    for g, sp in K.random_spellings():
        for s in sp[:2]:
            add(64, s)
    for s in S.mutated_rows(256) + [s for s, _ in S.MALFORMED_TABLE + S.OVERVALENT_TABLE]:
        add(64, s[:64])
    rng = random.Random(3)
    for s in SYMMETRIC:
        add(64, s)
        _, _, atoms, bonds = K.graph(s)
        to = list(range(len(atoms)))
        rng.shuffle(to)
        new = [0] * len(atoms)
        for a, d in enumerate(atoms):
            new[to[a]] = d
        moved = [(to[a], to[b], o) if rng.random() < 0.5 else (to[b], to[a], o) for a, b, o in bonds]
        rng.shuffle(moved)
        rows.append((64, len(new), len(moved), new, moved))
    rows += Q.edge_rows() + W.special_rows()
    with open(path, "w") as out:
        for width, n, nb, atoms, bonds in rows:
            out.write("T %d %d %d %d %d %s\n" % (width, n, nb, len(atoms), len(bonds), " ".join(map(str, list(atoms) + [N.pack(b) for b in bonds]))))
        for t, (width, n, nb, atoms, bonds) in enumerate(rows):
            r = Q.canon(n, atoms, nb, bonds, width)
            out.write("Q %d %d %d %s\n" % (t, r["flags"], -1 if r["flags"] == Q.UNDECIDED else r["nodes"],
                                           " ".join(map(str, r["priority"] + r["canon_atoms"] + r["canon_bonds"]))))


if __name__ == "__main__":
    main(sys.argv[1])
