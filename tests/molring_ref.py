"""Reference of mdt_mol_rings (csrc/k_molring.hip): the definition in include/mdt_hip.h in plain Python sets and ints on
molkey_ref.graph() and molh_ref's hydrogens, sharing no code and no table with the package.  Per bond entry the smallest cycle
through it (1 + a shortest path between its ends in the ring graph without that edge), per atom the smallest over its entries, and
per row the sixteen descriptors.  TABLE holds rows whose answers are written by hand."""
import molh_ref as H
import molkey_ref as K

MAX_WIDTH = 64
NAMES = ("heavy_atoms", "hetero_atoms", "donors", "acceptors", "rotatable_bonds", "rings", "ring_atoms", "ring_bonds", "smallest_ring",
         "largest_ring", "aromatic_atoms", "aromatic_outside_ring", "sp3_carbons", "carbons", "components", "weight")
MILLI = {"H": 1008, "B": 10810, "C": 12011, "N": 14007, "O": 15999, "F": 18998, "P": 30974, "S": 32060, "Cl": 35450, "Br": 79904,
         "I": 126904}                                                        # the eleven integers of the header comment
LIMIT_BIT = 128


def symbol_of(d):
    """descriptor -> the symbol with an upper-case first letter ('*' for the star)"""
    first, second = d & 31, d >> 5 & 31
    return "*" if first == 26 else chr(65 + first) + (chr(96 + second) if second else "")


def ring_graph(n, bonds):
    """-> {atom: set of neighbours} of the simple graph: distinct unordered pairs of distinct atoms, whatever the order"""
    adj = {a: set() for a in range(n)}
    for a, b, _ in bonds:
        if a != b:
            adj[a].add(b)
            adj[b].add(a)
    return adj


def shortest_without(adj, a, b):
    """the length of a shortest path from a to b that does not use the edge {a, b}, None if there is none"""
    dist, queue = {a: 0}, [a]
    while queue:
        x = queue.pop(0)
        for y in sorted(adj[x]):
            if {x, y} == {a, b} or y in dist:
                continue
            dist[y] = dist[x] + 1
            if y == b:
                return dist[y]
            queue.append(y)
    return None


def components_of(adj):
    left, count = set(adj), 0
    while left:
        stack = [min(left)]
        count += 1
        while stack:
            x = stack.pop()
            if x in left:
                left.discard(x)
                stack.extend(adj[x] & left)
    return count


def rings_arrays(n, atoms, nb, bonds, hydrogens, width=MAX_WIDTH):
    """-> dict(bond_ring [width], atom_ring [width], desc [16]) for a row of n atoms, nb bonds (a, b, order) and the hydrogens per
    atom; the counts are given apart from the lists so that arrays no scan writes can be asked about."""
    out = dict(bond_ring=[0] * width, atom_ring=[0] * width, desc=[0] * 16)
    if not H.is_graph(n, nb, bonds, width):
        return out
    atoms, bonds, hydrogens = list(atoms[:n]), list(bonds[:nb]), list(hydrogens[:n])
    adj = ring_graph(n, bonds)
    symbols = [symbol_of(d) for d in atoms]
    aromatic = [bool(d >> 10 & 1) for d in atoms]
    heavy = {a for a in range(n) if symbols[a] != "H"}
    for e, (a, b, _) in enumerate(bonds):
        if a != b:
            path = shortest_without(adj, a, b)
            out["bond_ring"][e] = 0 if path is None else 1 + path
    for a in range(n):
        sizes = [out["bond_ring"][e] for e, (x, y, _) in enumerate(bonds) if a in (x, y) and out["bond_ring"][e]]
        out["atom_ring"][a] = min(sizes, default=0)
    orders_at = [[o for x, y, o in bonds if a in (x, y)] for a in range(n)]
    turns = lambda a: len(adj[a] & heavy) >= 2 and not any(o in (3, 4) for o in orders_at[a])  # noqa: E731
    edges = sum(len(v) for v in adj.values()) // 2
    components = components_of(adj)
    sizes = [r for r in out["bond_ring"] if r]
    n_or_o = [s in ("N", "O") for s in symbols]
    weight = MILLI["H"] * sum(hydrogens) + sum(MILLI.get(s, 0) for s in symbols)
    out["desc"] = [
        len(heavy),
        sum(1 for a in heavy if symbols[a] != "C"),
        sum(1 for a in range(n) if n_or_o[a] and hydrogens[a] >= 1),
        sum(n_or_o),
        sum(1 for e, (a, b, o) in enumerate(bonds) if o == 1 and out["bond_ring"][e] == 0 and a != b and turns(a) and turns(b)),
        edges - n + components,
        sum(1 for a in range(n) if out["atom_ring"][a]),
        len(sizes),
        min(sizes, default=0),
        max(sizes, default=0),
        sum(aromatic),
        sum(1 for a in range(n) if aromatic[a] and not out["atom_ring"][a]),
        sum(1 for a in range(n) if symbols[a] == "C" and not aromatic[a] and all(o == 1 for o in orders_at[a])),
        sum(1 for s in symbols if s == "C"),
        components,
        weight]
    return out


def flag(desc, molecule, lo, hi):
    """the flag of the definition: 128 when the row is a molecule and some descriptor lies outside [lo, hi]; 0 without bounds"""
    if lo is None or not molecule:
        return 0
    return LIMIT_BIT if any(d < a or d > b for d, a, b in zip(desc, lo, hi)) else 0


_ROWS = {}


def string_rings(s, width=MAX_WIDTH):
    """The answer for a string (with `molecule`: is it a graph row at all?); one that is no molecule has no atoms."""
    at = (s, width)
    if at not in _ROWS:
        _, _, atoms, bonds = K.graph(s)
        hydrogens = H.string_hydrogens(s, H.MAX_STEPS, width)["hydrogens"]
        r = rings_arrays(len(atoms), atoms, len(bonds), bonds, hydrogens, width)
        r["molecule"] = H.is_graph(len(atoms), len(bonds), bonds, width)
        _ROWS[at] = r
    return _ROWS[at]


WIDEST_RING = "C1" + "C" * 60 + "C1"                                        # 64 tokens, 62 atoms: the deepest search
# string -> (bond_ring per entry in order of creation, atom_ring per atom in order of appearance, {descriptor: value}), all
# written by hand; a descriptor not named is not asserted
TABLE = {
    "C": ([], [0], dict(heavy_atoms=1, hetero_atoms=0, rings=0, components=1, sp3_carbons=1, carbons=1, weight=16043, rotatable_bonds=0)),
    "CC": ([0], [0, 0], dict(heavy_atoms=2, rings=0, rotatable_bonds=0, weight=30070, sp3_carbons=2)),
    "C1CC1": ([3, 3, 3], [3, 3, 3], dict(rings=1, ring_atoms=3, ring_bonds=3, smallest_ring=3, largest_ring=3, weight=42081)),
    "c1ccccc1": ([6] * 6, [6] * 6, dict(rings=1, ring_atoms=6, ring_bonds=6, smallest_ring=6, largest_ring=6, aromatic_atoms=6,
                                        aromatic_outside_ring=0, sp3_carbons=0, carbons=6, weight=78114, rotatable_bonds=0)),
    # naphthalene: atoms 3 and 8 are the fusion; the closure of ring 2 (entry 8) is the fusion bond, 6 like every other
    "c1ccc2ccccc2c1": ([6] * 11, [6] * 10, dict(rings=2, ring_atoms=10, ring_bonds=11, smallest_ring=6, largest_ring=6, aromatic_atoms=10,
                                                weight=128174)),
    "C1CC12CC2": ([3] * 6, [3] * 5, dict(rings=2, ring_atoms=5, ring_bonds=6, smallest_ring=3, largest_ring=3, components=1)),
    "C12C3C4C1C5C2C3C45": ([4] * 12, [4] * 8, dict(rings=5, ring_atoms=8, ring_bonds=12, smallest_ring=4, largest_ring=4, heavy_atoms=8,
                                                   weight=104152)),
    # norbornane: two five-rings over the one-carbon bridge; every bond lies in a five-ring
    "C1CC2CCC1C2": ([5] * 8, [5] * 7, dict(rings=2, ring_atoms=7, ring_bonds=8, smallest_ring=5, largest_ring=5, rotatable_bonds=0)),
    # biphenyl without '-': the inter-ring entry (entry 6, atoms 5 - 6, after the first ring's closure) is a bridge and, being
    # order 5, is not rotatable
    "c1ccccc1c1ccccc1": ([6] * 6 + [0] + [6] * 6, [6] * 12, dict(rings=2, rotatable_bonds=0, ring_bonds=12, aromatic_atoms=12)),
    "c1ccccc1-c1ccccc1": ([6] * 6 + [0] + [6] * 6, [6] * 12, dict(rings=2, rotatable_bonds=1, ring_bonds=12)),
    "CCCC": ([0, 0, 0], [0] * 4, dict(rotatable_bonds=1, rings=0, sp3_carbons=4, weight=58124)),
    "CC#CC": ([0, 0, 0], [0] * 4, dict(rotatable_bonds=0, sp3_carbons=2, carbons=4)),
    "CC(=O)NC": ([0] * 4, [0] * 5, dict(heavy_atoms=5, hetero_atoms=2, donors=1, acceptors=2, rotatable_bonds=1, sp3_carbons=2, carbons=3,
                                        weight=73095)),
    "C.C": ([], [0, 0], dict(components=2, rings=0, heavy_atoms=2, weight=32086)),
    "[Na+].[Cl-]": ([], [0, 0], dict(components=2, rings=0, heavy_atoms=2, hetero_atoms=2, weight=35450)),
    # the two closures name the same pair twice: one edge, one three-ring, both entries in it
    "C12CC12": ([3, 3, 3, 3], [3, 3, 3], dict(rings=1, ring_atoms=3, ring_bonds=4, smallest_ring=3, largest_ring=3)),
    "cc": ([0], [0, 0], dict(aromatic_atoms=2, aromatic_outside_ring=2, rings=0, weight=28054)),
    "[nH]1cccc1": ([5] * 5, [5] * 5, dict(donors=1, acceptors=1, hetero_atoms=1, rings=1, aromatic_atoms=5, weight=67091)),
    "CC(=O)O": ([0] * 3, [0] * 4, dict(donors=1, acceptors=2, hetero_atoms=2, rotatable_bonds=0, sp3_carbons=1, weight=60052)),
    "[2H]O[2H]": ([0, 0], [0] * 3, dict(heavy_atoms=1, hetero_atoms=1, donors=0, acceptors=1, weight=18015, components=1)),
    WIDEST_RING: ([62] * 62, [62] * 62, dict(rings=1, ring_atoms=62, ring_bonds=62, smallest_ring=62, largest_ring=62, heavy_atoms=62,
                                             rotatable_bonds=0, weight=62 * 14027)),
}
