#!/usr/bin/env python3
"""Writes the rows that tools/molmcs_host_check.cpp checks: graphs of the reference strings (tests/molkey_ref.py,
tests/smiles_ref.py), graph arrays that no scan writes, and for pairs of them every output word of tests/molmcs_ref.py with the
floor and every root's own size, step count and cap.

    python tools/molmcs_host_rows.py rows.txt

Lines: "G L n nb atoms_present bonds_present <atoms> <bond words>" (graph g, numbered as they come) and "P a b mode bonds atoms
bond_a steps flags out_natoms out_nbonds floor <LA map bytes> <LA atom words> <LA bond words> <LA atom_map bytes> roots <a0 b0 size
steps capped>...", sizes as bonds << 8 | atoms."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import molkey_ref as K  # noqa: E402
import molmcs_ref as C  # noqa: E402
import smiles_ref as S  # noqa: E402

CAP_A = "C(C)(C)(C)C(C)(C)C(C)(C)C(C)(C)C(C)(C)C(C)(C)C"
CAP_B = "CC(C)C(C)C(C)C(C)C(C)C(C)C(C)C"
SMALL = ["C1CC1C", "CC(C)(C)C", "C12CC1C2", "C12C3C1C23", "C.CO", "[NH3+]CC[O-]", "C1CC1", "CCC", "c1ccccc1O", "C1=CC=CC=C1", "CC(=O)O",
         "*C*", "N", "C#N"]


def word(bond):
    a, b, o = bond
    return a | b << 8 | o << 16


def main(path, graphs=40, wide=True):
    sys.setrecursionlimit(10000)
    pool, pairs = [], []                                                    # (width, n, nb, atoms, bonds (a, b, order))

    def add(width, s):
        atoms, bonds = C.graph_of(s)
        pool.append((width, len(atoms), len(bonds), atoms, bonds))
        return len(pool) - 1
    small = [add(len(s), s) for s in SMALL]
    pairs += [(a, b, mode) for a in small for b in small for mode in (0, 1)]
    for g, sp in K.random_spellings()[:graphs]:
        rows = [add(64, s) for s in sp[:2]]
        pairs += [(rows[0], rows[1], 1), (rows[1], rows[0], 0), (rows[0], small[len(pairs) % len(small)], 0)]
        if len(rows) > 1 and len(pool) > 20:
            pairs.append((rows[0], len(pool) - 4, 0))                        # against the graph before
    for s in S.mutated_rows(24):
        pairs += [(add(64, s[:64]), small[4], 0), (small[8], len(pool) - 1, 0)]
    if wide:
        pairs += [(add(64, CAP_A), add(64, CAP_B), 0), (add(64, "*" * 64), add(64, "*" * 64), 0),
                  (add(64, "C1" * 32), add(64, "C1CC1" * 12), 0), (add(1, "C"), add(1, "C"), 0), (add(1, "C"), add(1, "N"), 1)]
    # arrays that no scan writes, on either side
    c = K.descriptor("C")
    odd = [(8, 3, 2, [c] * 3, [(0, 3, 1), (1, 2, 1)]), (8, 9, 0, [], []), (8, 2, 9, [c] * 2, []), (8, -1, 0, [], []),
           (8, 2, -1, [c] * 2, []), (8, 2, 2, [c] * 2, [(0, 1, 1)] * 2), (8, 2, 1, [c] * 2, [(0, 0, 2)]),
           (8, 2, 1, [c] * 2, [(0, 1, 7)]), (8, 2, 2, [c] * 2, [(1, 1, 2), (1, 0, 1)]), (8, 3, 2, [c] * 3, [(0, 1, 1), (2, 1, 1)]),
           (8, 3, 4, [c] * 3, [(0, 1, 1), (1, 0, 1), (1, 2, 2), (2, 1, 1)])]
    first = len(pool)
    pool += odd
    pairs += [(a, b, 0) for a in range(first, len(pool)) for b in list(range(first, len(pool))) + small[:3]]
    pairs += [(small[1], b, 0) for b in range(first, len(pool))]
    with open(path, "w") as f:
        for width, n, nb, atoms, bonds in pool:
            f.write("G %d %d %d %d %d %s\n" % (width, n, nb, len(atoms), len(bonds),
                                               " ".join(map(str, list(atoms) + [word(b) for b in bonds]))))
        for a, b, mode in pairs:
            la, na, nba, a_atoms, a_bonds = pool[a]
            lb, nb, nbb, b_atoms, b_bonds = pool[b]
            w = C.mcs_arrays(na, a_atoms, nba, a_bonds, nb, b_atoms, nbb, b_bonds, mode, la, lb)
            f.write("P %d %d %d %d %d %d %d %d %d %d %d %s %d %s\n" % (
                a, b, mode, w["size"][0], w["size"][1], w["bond_a"], w["steps"], w["flags"], w["out_natoms"], w["out_nbonds"],
                w["floor"][0] << 8 | w["floor"][1],
                " ".join(map(str, w["map_a"] + w["out_atoms"] + w["out_bonds"] + w["atom_map"])), len(w["roots"]),
                " ".join("%d %d %d %d %d" % (a0, b0, bonds << 8 | atoms, steps, capped)
                         for a0, b0, bonds, atoms, steps, capped in w["roots"])))
    return len(pairs)


if __name__ == "__main__":
    main(sys.argv[1])
