#!/usr/bin/env python3
"""Writes the rows that tools/molwrite_host_check.cpp checks: the graphs of the reference strings (tests/molkey_ref.py,
tests/smiles_ref.py) as written, as normal forms (tests/molnorm_ref.py) and as scaffolds (tests/molscaf_ref.py), graph arrays that no
scan writes, and for each the answers of tests/molwrite_ref.py: the priority, and the written row with and without it at several
widths and under vocabularies that lack a class.

    python tools/molwrite_host_rows.py rows.txt

Lines: "C v <128 class_id bytes>" (vocabulary v), "T L n nb atoms_present bonds_present <atoms> <bond words>" (row t, numbered as
they come), "P t <L priority words>": mdt_mol_rank's answer for row t, "A t v invariant W length flags <W tokens> <W token_atom
bytes>": mdt_mol_write's answer for row t under vocabulary v, with the priority of "P t" (invariant 1) or without one (0)."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import molkey_ref as K  # noqa: E402
import molnorm_ref as N  # noqa: E402
import molscaf_ref as C  # noqa: E402
import molwrite_ref as W  # noqa: E402
import smiles_ref as S  # noqa: E402


def vocabularies():
    full = dict(W.ASCII)
    return [W.class_table(full), W.class_table({i: ch for i, ch in full.items() if ch != "%"}),
            W.class_table({i: ch for i, ch in full.items() if ch != "["}), W.class_table({i: ch for i, ch in full.items() if ch not in "(=1"})]


def main(path):
    rows = []

    def add(width, s, normalize=False):
        n, atoms, nb, bonds = C.input_arrays(s, normalize, width)
        rows.append((width, n, nb, atoms, bonds))
    for s in list(C.TABLE) + list(N.TABLE):
        add(64, s), add(64, s, True)
        add(max(1, len(s)), s)                                               # as narrow as the string
        for mode in C.MODES:
            r = C.string_scaffold(s, mode, True)                             # the scaffold of the normal form
            rows.append((64, r["n"], r["nb"]) + C.unpacked(r))
    for g, sp in K.random_spellings():
        for s in sp[:2]:
            add(64, s)
        add(64, sp[0], True)
    for s in S.mutated_rows(256) + [s for s, _ in S.MALFORMED_TABLE + S.OVERVALENT_TABLE]:
        add(64, s[:64])
    for s in ("C" * 64, "c" * 64, "c1ccccc1" * 8, "*" * 64, "", "C(", "C1CC1" + "C" * 59, "C1" + "C" * 60 + "C1", "C1CC1" + "C" * 54 + "C1CC1",
              "C12C3C4C1C5C2C3C45", "C12C3C4C1C5C2C3C45.C12C3C4C1C5C2C3C45", "c1cc2ccc3cccc4ccc(c1)c2c34", "O=C1C(=O)C(=O)C1=O",
              "[13CH3]C", "[NH4+].[Cl-]", "C%12CCCCC%12"):
        add(64, s)
    rows += W.special_rows()
    tables = vocabularies()
    with open(path, "w") as out:
        for v, table in enumerate(tables):
            out.write("C %d %s\n" % (v, " ".join(map(str, table))))
        for width, n, nb, atoms, bonds in rows:
            out.write("T %d %d %d %d %d %s\n" % (width, n, nb, len(atoms), len(bonds), " ".join(map(str, list(atoms) + [N.pack(b) for b in bonds]))))
        for t, (width, n, nb, atoms, bonds) in enumerate(rows):
            prio = W.priority(n, atoms, nb, bonds, width)
            out.write("P %d %s\n" % (t, " ".join(map(str, prio))))
            full = W.write_arrays(n, atoms, nb, bonds, prio, tables[0], 128, width)
            T = full["length"]
            asked = [(0, 1, 128), (0, 0, 64), (1, 1, 64), (2, 0, 128), (3, 1, 128)]
            asked += [(0, 1, w) for w in {max(1, T - 1), max(1, T), 1} if w <= 128]
            for v, invariant, width_out in asked:
                r = W.write_arrays(n, atoms, nb, bonds, prio if invariant else None, tables[v], width_out, width)
                out.write("A %d %d %d %d %d %d %s\n" % (t, v, invariant, width_out, r["length"], r["flags"],
                                                       " ".join(map(str, r["tokens"] + r["token_atom"]))))


if __name__ == "__main__":
    main(sys.argv[1])
