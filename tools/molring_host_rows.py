#!/usr/bin/env python3
"""Writes the rows that tools/molring_host_check.cpp checks: the graphs of the reference strings (tests/molkey_ref.py,
tests/smiles_ref.py) with the hydrogens of tests/molh_ref.py, graph arrays that no scan writes, and for each the answer of
tests/molring_ref.py, without bounds and under bounds.

    python tools/molring_host_rows.py rows.txt

Lines: "T L n nb atoms_present bonds_present <atoms> <bond words> <atoms_present hydrogens>" (row t, numbered as they come),
"A t bounded flag <16 lo> <16 hi> <L bond_ring> <L atom_ring> <16 descriptors>": the answer for row t; with bounded == 0 the bounds
are not handed over (and are written as zeros)."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import molh_ref as H  # noqa: E402
import molkey_ref as K  # noqa: E402
import molring_ref as R  # noqa: E402
import smiles_ref as S  # noqa: E402

LOW, HIGH = -2 ** 31, 2 ** 31 - 1


def word(bond):
    a, b, o = bond
    return a | b << 8 | o << 16


def bounds(**named):
    lo, hi = [LOW] * 16, [HIGH] * 16
    for key, value in named.items():
        (lo if key[:3] == "min" else hi)[R.NAMES.index(key[4:])] = value
    return lo, hi


BOUNDS = [bounds(max_rings=0), bounds(min_smallest_ring=5), bounds(max_weight=100000, max_donors=0), bounds(min_components=2),
          bounds(max_largest_ring=5, min_heavy_atoms=4), bounds()]


def main(path):
    rows = []                                                                # (width, n, nb, atoms, bonds (a, b, order), hydrogens)

    def add(width, s):
        _, _, atoms, bonds = K.graph(s)
        hydrogens = H.string_hydrogens(s, H.MAX_STEPS, 64)["hydrogens"][:len(atoms)]
        rows.append((width, len(atoms), len(bonds), atoms, bonds, hydrogens))
    for s in R.TABLE:
        add(64, s)
        add(max(1, len(s)), s)                                               # as narrow as the string
    for g, sp in K.random_spellings():
        for s in sp:
            add(64, s)
    for s in S.mutated_rows(512) + [s for s, _ in S.MALFORMED_TABLE + S.OVERVALENT_TABLE]:
        add(64, s[:64])
    for s in ("C" * 64, "c" * 64, "c1ccccc1" * 8, "*" * 64, "", "C(", "C1C2C3C4C5C6C7C8C9C%10C%11C%12C%13C%14C%15C1C2C3",
              "C%10CCC(CC%10)C%11CCC(CC%11)C%12CCC(CC%12)C%13CCC(CC%13)C1CCCCC1"):
        add(64, s)
    # arrays that no scan writes: counts outside [0, width], a bond naming a missing atom, an order outside 1..5, a bond listed
    # twice, a bond of an atom to itself, a complete graph, hydrogens no rule gives
    c, n_, h = K.descriptor("C"), K.descriptor("N"), K.descriptor("H", True)
    k8 = [(i, j, 1) for i in range(8) for j in range(i)]
    for row in [(8, 3, 2, [c] * 3, [(0, 3, 1), (1, 2, 1)], [0] * 3), (8, 9, 0, [], [], []), (8, 2, 9, [c] * 2, [], [0] * 2),
                (8, -1, 0, [], [], []), (8, 2, -1, [c] * 2, [], [0] * 2), (8, 0, 0, [], [], []),
                (8, 3, 4, [c] * 3, [(0, 1, 1), (1, 0, 1), (1, 2, 1), (2, 0, 1)], [2] * 3),
                (8, 3, 3, [c] * 3, [(0, 0, 1), (0, 1, 1), (1, 2, 3)], [1, 2, 3]), (8, 2, 1, [c] * 2, [(0, 1, 7)], [0, 0]),
                (8, 4, 4, [c, n_, c, c], [(0, 1, 0), (1, 2, 65535), (2, 3, 1), (3, 0, 1)], [255, 255, 0, 1]),
                (28, 8, 28, [c] * 8, k8, [0] * 8), (4, 4, 3, [h, n_, h, c], [(0, 1, 1), (1, 2, 1), (1, 3, 1)], [0, 0, 0, 3]),
                (1, 1, 1, [c], [(0, 0, 1)], [4]), (1, 1, 0, [n_], [], [3]),
                (64, 64, 64, [c] * 64, [(i, (i + 1) % 64, 1) for i in range(64)], [2] * 64)]:
        rows.append(row)
    with open(path, "w") as out:
        for width, n, nb, atoms, bonds, hydrogens in rows:
            assert len(hydrogens) == len(atoms)
            out.write("T %d %d %d %d %d %s\n" % (width, n, nb, len(atoms), len(bonds),
                                                " ".join(map(str, list(atoms) + [word(b) for b in bonds] + list(hydrogens)))))
        for t, (width, n, nb, atoms, bonds, hydrogens) in enumerate(rows):
            r = R.rings_arrays(n, list(atoms), nb, list(bonds), list(hydrogens), width)
            molecule = H.is_graph(n, nb, bonds, width)
            asks = [(0, [0] * 16, [0] * 16)] + [(1, lo, hi) for lo, hi in (BOUNDS if t % 7 == 0 or t >= len(rows) - 15 else BOUNDS[t % 6:t % 6 + 1])]
            for bounded, lo, hi in asks:
                flag = R.flag(r["desc"], molecule, lo, hi) if bounded else 0
                out.write("A %d %d %d %s\n" % (t, bounded, 1 if flag else 0,
                                               " ".join(map(str, lo + hi + r["bond_ring"] + r["atom_ring"] + r["desc"]))))


if __name__ == "__main__":
    main(sys.argv[1])
