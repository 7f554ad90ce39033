"""Reference of mdt_mol_normalize (csrc/k_molnorm.hip): the definition in include/mdt_hip.h in plain Python sets and ints on
molkey_ref.graph(), molh_ref's hydrogens and Kekule structure and molring_ref's ring sizes, sharing no code and no table with the
package.  Per row the normal form of the graph -- one set of arrays for the Kekule, the aromatic and the bracket spelling of a
molecule -- and its flags.  TABLE holds rows whose aromatic atoms are written by hand."""
import molh_ref as H
import molkey_ref as K
import molring_ref as R

MAX_WIDTH = 64
NORMALIZED, AROMATIC, CHANGED = 1, 2, 4                                      # the flag bits
GROUP = {"B": 13, "C": 14, "N": 15, "P": 15, "O": 16, "S": 16}               # every other symbol is ineligible


def pack(bond):
    a, b, o = bond
    return a | b << 8 | o << 16


def kekule_orders(bonds, partner):
    """the Kekule view: an entry of order 5 is 2 where its two ends are each other's partner, 1 otherwise"""
    return [o if o != 5 else (2 if a != b and partner[a] == 1 + b and partner[b] == 1 + a else 1) for a, b, o in bonds]


def pi_electrons(n, atoms, bonds, k, hydrogens, bond_ring):
    """-> [p or None per atom]: what the atom gives to a ring's pi system, None for an atom that can be in no aromatic ring"""
    out = []
    for x in range(n):
        symbol, _, _, charge, _ = H.fields(atoms[x])
        at = [e for e, (a, b, _) in enumerate(bonds) if x in (a, b)]
        proper = [e for e in at if bonds[e][0] != bonds[e][1]]
        double = [e for e in proper if k[e] == 2]
        sigma = len(proper) + hydrogens[x]
        p = None
        if symbol in GROUP and not any(k[e] in (3, 4) for e in at) and len(double) <= 1:
            g = GROUP[symbol] - charge
            if double:
                e = double[0]
                other = bonds[e][0] + bonds[e][1] - x
                if bond_ring[e]:
                    p = 1
                elif symbol == "C" and charge == 0 and H.fields(atoms[other])[0] in ("N", "O", "S"):
                    p = 0
            elif (g == 16 and sigma == 2) or (g == 15 and sigma == 3):
                p = 2
            elif g == 13 and sigma == 3:
                p = 0
        out.append(p)
    return out


def two_rings(adj, a, b):
    """The two rings tried for the entry (a, b): breadth first from a to b without the edge {a, b}, every atom keeping the level at
    which it was reached, then back from b taking at every level the lowest-numbered predecessor, and again the highest.
    -> [frozenset, frozenset] (equal when there is one), [] when b is not reached."""
    level, frontier, depth = {a: 0}, {a}, 0
    while b not in level:
        depth += 1
        found = set()
        for x in frontier:
            for y in adj[x]:
                if {x, y} != {a, b} and y not in level:
                    found.add(y)
        if not found:
            return []
        for y in found:
            level[y] = depth
        frontier = found
    rings = []
    for pick in (min, max):
        ring, at = {a, b}, b
        for lvl in range(level[b] - 1, 0, -1):
            at = pick(x for x in adj[at] if level.get(x) == lvl)
            ring.add(at)
        rings.append(frozenset(ring))
    return rings


def normalize_arrays(n, atoms, nb, bonds, hydrogens, partner, verdict, bond_ring, width=MAX_WIDTH):
    """-> dict(atoms [width] ints, bonds [width] packed words, flags, aromatic: the set of aromatic atoms, tried: the rings tried,
    rings: those that passed) for a row of n atoms, nb bonds (a, b, order), with the outputs of mdt_mol_hydrogens and mdt_mol_rings
    for it.  The counts are given apart from the lists so that arrays no scan writes can be asked about."""
    out = dict(atoms=[0] * width, bonds=[0] * width, flags=0, aromatic=set(), tried=[], rings=[])
    if not H.is_graph(n, nb, bonds, width):
        return out
    atoms, bonds = list(atoms[:n]), list(bonds[:nb])
    if verdict != 0:                                                         # as written
        out["atoms"][:n], out["bonds"][:nb] = atoms, [pack(e) for e in bonds]
        return out
    k = kekule_orders(bonds, partner)
    p = pi_electrons(n, atoms, bonds, k, hydrogens, bond_ring)
    adj = R.ring_graph(n, bonds)
    order = list(k)
    for e, (a, b, _) in enumerate(bonds):
        if a == b or not bond_ring[e] or p[a] is None or p[b] is None:
            continue
        for ring in two_rings(adj, a, b):
            if ring not in out["tried"]:
                out["tried"].append(ring)
            if all(p[x] is not None for x in ring) and sum(p[x] for x in ring) % 4 == 2 and ring not in out["rings"]:
                out["rings"].append(ring)
    for ring in out["rings"]:
        out["aromatic"] |= ring
        for e, (a, b, _) in enumerate(bonds):
            if a in ring and b in ring:
                order[e] = 5
    flags = NORMALIZED | (AROMATIC if out["rings"] else 0)
    for x in range(n):
        d = atoms[x]
        out["atoms"][x] = (d & ~(1 << 10 | 15 << 17)) | 1 << 11 | (int(x in out["aromatic"]) << 10) | min(hydrogens[x], 15) << 17
        if bool(d >> 10 & 1) != (x in out["aromatic"]):
            flags |= CHANGED
    for e, (a, b, o) in enumerate(bonds):
        out["bonds"][e] = pack((a, b, order[e]))
        if order[e] != o:
            flags |= CHANGED
    out["flags"] = flags
    return out


_ROWS = {}


def string_normal(s, width=MAX_WIDTH):
    """The answer for a string, with `n`, `nb`, `molecule` (is it a graph row at all?) and `verdict`."""
    at = (s, width)
    if at not in _ROWS:
        _, _, atoms, bonds = K.graph(s)
        h = H.string_hydrogens(s, H.MAX_STEPS, width)
        r = R.string_rings(s, width)
        out = normalize_arrays(len(atoms), atoms, len(bonds), bonds, h["hydrogens"], h["partner"], h["verdict"], r["bond_ring"], width)
        out.update(n=len(atoms), nb=len(bonds), molecule=r["molecule"], verdict=h["verdict"])
        _ROWS[at] = out
    return _ROWS[at]


def unpacked(out):
    """(atoms, bonds as (a, b, order)) of an answer, cut to its counts: what molkey_ref.key() takes"""
    return out["atoms"][:out["n"]], [(w & 255, w >> 8 & 255, w >> 16) for w in out["bonds"][:out["nb"]]]


def normal_key(s):
    """molkey_ref's key of the normal form of a string (0: no molecule)"""
    out = string_normal(s)
    return K.key(*unpacked(out)) if out["molecule"] else 0


def again(out):
    """The normal form of a normal form: hydrogens, Kekule structure and ring sizes are computed afresh on its arrays."""
    atoms, bonds = unpacked(out)
    n, nb = len(atoms), len(bonds)
    h = H.hydrogens_arrays(n, atoms, nb, bonds)
    r = R.rings_arrays(n, atoms, nb, bonds, h["hydrogens"])
    new = normalize_arrays(n, atoms, nb, bonds, h["hydrogens"], h["partner"], h["verdict"], r["bond_ring"])
    new.update(n=n, nb=nb, molecule=True, verdict=h["verdict"])
    return new


def kekule_string_arrays(s):
    """The Kekule view of a string as graph arrays: its atoms with bit 10 cleared, its entries at their Kekule orders."""
    _, _, atoms, bonds = K.graph(s)
    h = H.string_hydrogens(s)
    k = kekule_orders(bonds, h["partner"])
    return [d & ~(1 << 10) for d in atoms], [(a, b, o) for (a, b, _), o in zip(bonds, k)], h["hydrogens"]


def arrays_row(width, n, atoms, nb, bonds, **given):
    """A row handed over as arrays -> (width, n, nb, atoms, bonds, hydrogens, partner, verdict, bond_ring): what the references of
    mdt_mol_hydrogens and mdt_mol_rings say about it, each replaced by what `given` names."""
    h = H.hydrogens_arrays(n, list(atoms), nb, list(bonds), width)
    row = dict(hydrogens=h["hydrogens"][:len(atoms)], partner=h["partner"][:len(atoms)], verdict=h["verdict"])
    row.update({k: v for k, v in given.items() if k != "bond_ring"})
    ring = R.rings_arrays(n, list(atoms), nb, list(bonds), row["hydrogens"], width)["bond_ring"][:len(bonds)]
    return (width, n, nb, list(atoms), list(bonds), list(row["hydrogens"]), list(row["partner"]), row["verdict"],
            list(given.get("bond_ring", ring)))


def special_rows():
    """Graph arrays that no scan writes, with what is expected of some of them: [(row of arrays_row, {what: value})]."""
    c, n_, o_ = K.descriptor("C"), K.descriptor("N"), K.descriptor("O")
    alternating = lambda m: [(i, (i + 1) % m, 2 if i % 2 == 0 else 1) for i in range(m)]  # noqa: E731
    benzene = alternating(6)
    rows = [
        # a 62-ring of alternating bonds with two substituents, n = 64: 62 electrons, 2 mod 4, 31 search levels
        (arrays_row(64, 64, [c] * 64, 64, alternating(62) + [(0, 62, 1), (31, 63, 1)]), dict(aromatic=set(range(62)), flags=7)),
        (arrays_row(64, 64, [c] * 64, 64, alternating(64)), dict(aromatic=set(), flags=1)),          # 64 electrons: 0 mod 4
        (arrays_row(8, 6, [c] * 6, 7, benzene + [(1, 2, 1)]), dict(aromatic=set(range(6)), flags=7)),   # a single entry listed twice
        (arrays_row(8, 6, [c] * 6, 7, benzene + [(0, 1, 2)], hydrogens=[1] * 6), dict(aromatic=set(), flags=1)),   # a double one: dbl == 2
        (arrays_row(8, 6, [c] * 6, 7, benzene + [(0, 0, 1)], hydrogens=[1] * 6), dict(aromatic=set(range(6)), flags=7)),   # (x, x): order 5
        (arrays_row(8, 6, [c] * 6, 7, benzene + [(3, 3, 3)], hydrogens=[1] * 6), dict(aromatic=set(), flags=1)),   # (x, x) of order 3
        (arrays_row(1, 1, [c], 0, [], hydrogens=[200]), dict(flags=1)),                                # the H field clamps at 15
        (arrays_row(4, 2, [c, o_], 1, [(0, 1, 2)], hydrogens=[255, 16]), dict(flags=1)),
        (arrays_row(8, 2, [c, c], 1, [(0, 1, 2)], bond_ring=[3]), dict(aromatic=set(), flags=1)),     # a ring bond the search cannot close
        (arrays_row(8, 4, [c, n_, c, c], 4, [(0, 1, 0), (1, 2, 65535), (2, 3, 1), (3, 0, 1)]), dict(aromatic=set(), flags=1)),
        (arrays_row(8, 6, [c] * 6, 6, benzene, verdict=2), dict(flags=0)),                             # verdict != 0: as written
        (arrays_row(8, 6, [c] * 6, 6, benzene, verdict=3, hydrogens=[9] * 6, partner=[2, 1, 4, 3, 6, 5]), dict(flags=0)),
        # counts outside the row (whatever its width), a bond naming a missing atom: no molecule
        (arrays_row(8, 65, [], 0, []), dict(flags=0)), (arrays_row(8, 2, [c] * 2, 65, []), dict(flags=0)),
        (arrays_row(8, -1, [], 0, []), dict(flags=0)), (arrays_row(8, 2, [c] * 2, -1, []), dict(flags=0)),
        (arrays_row(8, 0, [], 0, []), dict(flags=0)), (arrays_row(8, 3, [c] * 3, 2, [(0, 3, 1), (1, 2, 1)]), dict(flags=0)),
        # the complete graph on 8 atoms: every bond in many triangles
        (arrays_row(28, 8, [c] * 8, 28, [(i, j, 1) for i in range(8) for j in range(i)]), dict(aromatic=set(), flags=1)),
    ]
    return rows


def special_answer(row):
    width, n, nb, atoms, bonds, hydrogens, partner, verdict, bond_ring = row
    return normalize_arrays(n, atoms, nb, bonds, hydrogens, partner, verdict, bond_ring, width)


ALL = "all"
# string -> the aromatic atoms (indices in order of appearance; ALL: every atom), written by hand
TABLE = {
    # every ring atom is aromatic
    "c1ccccc1": ALL, "C1=CC=CC=C1": ALL,
    "c1ccncc1": ALL, "C1=CC=NC=C1": ALL,
    "c1cc[nH]c1": ALL, "C1=CNC=C1": ALL,
    "c1ccoc1": ALL, "C1=COC=C1": ALL,
    "c1c[nH]cn1": ALL, "C1=CNC=N1": ALL,
    "c1ccsc1": ALL,
    "c1ccc2ccccc2c1": ALL, "C1=CC2=C(C=C1)C=CC=C2": ALL, "C1=CC=C2C=CC=CC2=C1": ALL, "C1=CC2=CC=CC=C2C=C1": ALL,
    "c1ccc2[nH]ccc2c1": ALL, "C1=CC=C2NC=CC2=C1": ALL,
    "[CH+]1C=CC=CC=C1": ALL, "c1ccc[cH+]cc1": ALL,
    "[CH-]1C=CC=C1": ALL, "C1=C[CH+]1": ALL,
    "c1ccccc1c1ccccc1": ALL, "C1=CC=CC=C1C1=CC=CC=C1": ALL,
    # only part of the molecule is aromatic
    "O=c1cc[nH]cc1": {1, 2, 3, 4, 5, 6}, "O=C1C=CNC=C1": {1, 2, 3, 4, 5, 6},
    "Cn1cnc2c1c(=O)n(C)c(=O)n2C": {1, 2, 3, 4, 5, 6, 8, 10, 12}, "CN1C=NC2=C1C(=O)N(C)C(=O)N2C": {1, 2, 3, 4, 5, 6, 8, 10, 12},
    "[O-][n+]1ccccc1": {1, 2, 3, 4, 5, 6},
    "c1ccc2CCCCc2c1": {0, 1, 2, 3, 8, 9},
    "c1ccc2c(c1)Cc1ccccc12": set(range(13)) - {6},
    # nothing is aromatic
    "O=C1C=CC(=O)C=C1": set(), "C1=CC=CC=CC=C1": set(), "C1=CC=C1": set(), "c1ccc1": set(), "C1=CCC=C1": set(),
    "c1ccc2cccc2cc1": set(),                                                 # azulene: no envelope rings
    "cc": set(), "C1CCCCC1": set(),
}
# two spellings of one molecule whose keys as written differ and whose normal forms have one key
PAIRS = [("[CH4]", "C"), ("c1ccccc1", "C1=CC=CC=C1"), ("CC1=C(O)C=CC=C1", "CC=1C(O)=CC=CC=1"),
         ("Cn1cnc2c1c(=O)n(C)c(=O)n2C", "CN1C=NC2=C1C(=O)N(C)C(=O)N2C"), ("c1ccc2[nH]ccc2c1", "C1=CC=C2NC=CC2=C1"),
         ("O=c1cc[nH]cc1", "O=C1C=CNC=C1"), ("c1ccc[cH+]cc1", "[CH+]1C=CC=CC=C1"), ("c1ccccc1c1ccccc1", "C1=CC=CC=C1C1=CC=CC=C1"),
         ("c1ccc2ccccc2c1", "C1=CC2=C(C=C1)C=CC=C2"), ("[OH2]", "O"), ("C[NH2]", "CN")]
