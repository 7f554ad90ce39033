#!/usr/bin/env python3
"""Writes the rows that tools/molmap_host_check.cpp checks: target and pattern graphs of the reference strings (tests/molkey_ref.py,
tests/smiles_ref.py), graph arrays that no scan writes, and for (target, pattern) pairs every output word of tests/molmap_ref.py
with every root's own embeddings and step count.

    python tools/molmap_host_rows.py rows.txt

Lines: "T L n nb atoms_present bonds_present <atoms> <bond words>" (target t, numbered as they come), "Q LP m mb atoms_present
bonds_present <atoms> <bond words>" (pattern q), "M t q found capped embeddings cover <LP map bytes> roots <root seen steps>..."."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import molkey_ref as K  # noqa: E402
import molmap_ref as A  # noqa: E402
import molsub_ref as B  # noqa: E402
import smiles_ref as S  # noqa: E402

CAP_PATTERN = "C.C.C.C.C.C.CN"


def word(bond):
    a, b, o = bond
    return a | b << 8 | o << 16


def main(path, graphs=120):
    spelled = K.random_spellings()[:graphs]
    targets, patterns, pairs = [], [], []                                   # (width, n, nb, atoms, bonds (a, b, order))

    def add(pool, width, s):
        atoms, bonds = B.graph_of(s)
        pool.append((width, len(atoms), len(bonds), atoms, bonds))
        return len(pool) - 1
    small = [add(patterns, 32, p) for p in B.PATTERNS]
    for g, sp in spelled:
        rows = [add(targets, 64, s) for s in sp[:2]]
        pairs += [(t, q) for t in rows for q in small]
        if len(sp[0]) <= 32:                                                 # a molecule in another spelling of itself
            pairs.append((rows[-1], add(patterns, 32, sp[0])))
    for s in S.mutated_rows(128) + [s for s, _ in S.MALFORMED_TABLE + S.OVERVALENT_TABLE]:
        t = add(targets, 64, s[:64])
        pairs += [(t, q) for q in small[:12]]
    wide_p = [add(patterns, 32, p) for p in ("C" * 32, "*" * 32, "c1ccccc1c1ccccc1", "C1CCCCCCCCCCCCCCC1", "C(C)(C)C", "*.*.*.*",
                                             CAP_PATTERN, "C(C1)1", "N", "NC")]
    for s in ("C" * 64, "C1C2C3C4C5C6C7C8C9C%10C%11C%12C%13C%14C%15C1C2C3", "C1" * 32, "c1ccccc1" * 8, "*" * 64, "", "C(",
              "C" * 62 + ".N", "C" * 61 + "CN", "C1CC1", "N" + "C" * 63, "C" * 63 + "N", "C" * 40 + "N"):
        t = add(targets, 64, s)
        pairs += [(t, q) for q in wide_p + small]
    pairs += [(add(targets, 1, "C"), q) for q in small[:4]] + [(add(targets, 3, "OCO"), add(patterns, 1, "O"))]     # the narrowest arrays
    # arrays that no scan writes, on either side
    c = K.descriptor("C")
    odd = [(8, 3, 2, [c] * 3, [(0, 3, 1), (1, 2, 1)]), (8, 9, 0, [], []), (8, 2, 9, [c] * 2, []), (8, -1, 0, [], []),
           (8, 2, -1, [c] * 2, []), (8, 2, 2, [c] * 2, [(0, 1, 1)] * 2), (8, 2, 1, [c] * 2, [(0, 0, 2)]),
           (8, 2, 1, [c] * 2, [(0, 1, 7)]), (8, 2, 2, [c] * 2, [(1, 1, 2), (1, 0, 1)]), (8, 3, 2, [c] * 3, [(0, 1, 1), (2, 1, 1)])]
    odd_t, odd_q = [], []
    for row in odd:
        targets.append(row)
        patterns.append(row)
        odd_t.append(len(targets) - 1)
        odd_q.append(len(patterns) - 1)
    pairs += [(t, q) for t in odd_t for q in odd_q + small[:3]] + [(add(targets, 64, "CC(C)C"), q) for q in odd_q]
    with open(path, "w") as f:
        for tag, pool in (("T", targets), ("Q", patterns)):
            for width, n, nb, atoms, bonds in pool:
                f.write("%s %d %d %d %d %d %s\n" % (tag, width, n, nb, len(atoms), len(bonds),
                                                    " ".join(map(str, list(atoms) + [word(b) for b in bonds]))))
        for t, q in pairs:
            L, n, nb, atoms, bonds = targets[t]
            LP, m, mb, p_atoms, p_bonds = patterns[q]
            w = A.map_arrays(n, atoms, nb, bonds, m, p_atoms, mb, p_bonds, L, LP)
            f.write("M %d %d %d %d %d %d %s %d %s\n" % (t, q, w["found"], w["capped"], w["embeddings"], w["cover"],
                                                        " ".join(map(str, w["map"])), len(w["roots"]),
                                                        " ".join("%d %d %d" % (r, seen, steps) for r, seen, _, steps in w["roots"])))
    return len(pairs)


if __name__ == "__main__":
    main(sys.argv[1])
