"""Reference of mdt_mol_mcs (csrc/k_molmcs.hip): the definition in include/mdt_hip.h in plain Python ints on molkey_ref.graph(),
sharing no code and no table with the package.  Three things: the WALK of one root, recursive as the header writes it (the kernel
keeps a stack of bytes and computes the rest again on the way back); the PAIR (greedy floor, roots, winner, recount, flags, the
graph arrays); and an INDEPENDENT brute force that knows nothing of roots, bounds or steps -- every connected entry subset of A
under every injective image."""
import itertools

import molkey_ref as K

MAX_STEPS, MAX_WIDTH = 4096, 64
EXACT_ATOMS = 1
PAIR, COMMON, UNDECIDED, WHOLE_A, WHOLE_B = 1, 2, 4, 8, 16


class Capped(Exception):
    pass


def is_graph(n, nb, bonds, width):
    """The rule of mdt_mol_key: counts inside [1, width] x [0, width], every bond end below n."""
    return 1 <= n <= width and 0 <= nb <= width and all(a < n and b < n for a, b, _ in bonds[:nb])


def usable(entry):
    a, b, o = entry
    return a != b and 1 <= o <= 5


def compatible(x, y, mode):
    return x == y if mode & EXACT_ATOMS else (x ^ y) & 0x7FF == 0


def lowest(w):
    return (w & -w).bit_length() - 1


def bits(w):
    return bin(w).count("1")


class Tables:
    """What a pair's roots share: A's entries, B's adjacency words per order, compat."""

    def __init__(self, a_atoms, a_bonds, b_atoms, b_bonds, mode):
        self.na, self.nb = len(a_atoms), len(b_atoms)
        self.entries = list(a_bonds)
        self.adj_b = [[0] * self.nb for _ in range(6)]
        for a, b, o in b_bonds:
            if usable((a, b, o)):
                self.adj_b[o][a] |= 1 << b
                self.adj_b[o][b] |= 1 << a
        self.total_b = [sum(bits(w) for w in self.adj_b[o]) // 2 for o in range(6)]
        self.compat = [sum(1 << t for t in range(self.nb) if compatible(a_atoms[a], b_atoms[t], mode)) for a in range(self.na)]
        self.at = [[k for k, e in enumerate(self.entries) if usable(e) and a in e[:2]] for a in range(self.na)]


class Root:
    """The walk of root (a0, b0).  After walk(): best (bonds, atoms), best_map {a: t}, steps, capped."""

    def __init__(self, t, a0, b0, floor=(0, 0), cap=MAX_STEPS):
        self.t, self.a0, self.floor, self.cap = t, a0, floor, cap
        self.m, self.used, self.x, self.cur = {a0: b0}, 1 << b0, set(), 0
        self.best, self.best_map, self.steps, self.capped = (-1, 0), None, 0, False
        self.live = [k for k, e in enumerate(t.entries) if usable(e) and e[0] >= a0 and e[1] >= a0]

    def bound(self):
        t, m = self.t, self.m
        ub = self.cur
        for o in range(1, 6):
            ra = sum(1 for k in self.live if t.entries[k][2] == o and k not in self.x
                     and not (t.entries[k][0] in m and t.entries[k][1] in m))
            inside = sum(bits(t.adj_b[o][u] & self.used) for u in range(t.nb) if self.used >> u & 1) // 2
            ub += min(ra, t.total_b[o] - inside)
        free = sum(1 for a in range(self.a0, t.na) if a not in m)
        return ub, len(m) + min(free, t.nb - len(m))

    def pick(self):
        """Step 3 -> (entry index, mapped end, free end, candidate word) or None."""
        t, m = self.t, self.m
        for k in self.live:
            a, b, o = t.entries[k]
            if k in self.x or (a in m) == (b in m):
                continue
            x, y = (a, b) if a in m else (b, a)
            c = t.adj_b[o][m[x]] & t.compat[y] & ~self.used
            if c:
                return k, x, y, c
        return None

    def assign(self, y, at):
        """M(y) = at -> the entries counted: those at y, not excluded, whose other end is mapped onto a neighbour of at."""
        t, m = self.t, self.m
        gained = 0
        for k in t.at[y]:
            a, b, o = t.entries[k]
            z = b if a == y else a
            if k not in self.x and z in m and t.adj_b[o][at] >> m[z] & 1:
                gained += 1
        m[y] = at
        self.used |= 1 << at
        self.cur += gained
        return gained

    def undo(self, y, at, gained):
        del self.m[y]
        self.used &= ~(1 << at)
        self.cur -= gained

    def step(self):
        if self.steps == self.cap:
            raise Capped
        self.steps += 1

    def node(self):
        size = (self.cur, len(self.m))
        if size > self.best:
            self.best, self.best_map = size, dict(self.m)
        ub = self.bound()
        if ub <= self.best or ub < self.floor:
            return
        picked = self.pick()
        if picked is None:
            return
        k, _, y, c = picked
        while c:
            at = lowest(c)
            c &= c - 1
            self.step()
            gained = self.assign(y, at)
            self.node()
            self.undo(y, at, gained)
        self.step()
        self.x.add(k)
        self.node()
        self.x.discard(k)

    def walk(self):
        try:
            self.node()
        except Capped:
            self.capped = True
        return self

    def greedy(self):
        """The greedy descent -> the size it reaches.  No step is counted."""
        while True:
            picked = self.pick()
            if picked is None:
                return self.cur, len(self.m)
            _, _, y, c = picked
            self.assign(y, lowest(c))


def recount(t, m):
    """The matched A entries under the map m -> the bond mask."""
    mask = 0
    for k, (a, b, o) in enumerate(t.entries):
        if usable((a, b, o)) and a in m and b in m and t.adj_b[o][m[a]] >> m[b] & 1:
            mask |= 1 << k
    return mask


def mcs_arrays(na, a_atoms, nba, a_bonds, nb, b_atoms, nbb, b_bonds, mode=0, la=MAX_WIDTH, lb=MAX_WIDTH, cap=MAX_STEPS,
               use_floor=True):
    """-> dict of every output word of one pair, and roots: [(a0, b0, bonds, atoms, steps, capped)]"""
    out = dict(size=(0, 0), map_a=[0] * la, bond_a=0, steps=0, flags=0, out_natoms=0, out_atoms=[0] * la, out_nbonds=0,
               out_bonds=[0] * la, atom_map=[0] * la, roots=[], floor=(0, 0), search_size=(0, 0))
    if not is_graph(na, nba, a_bonds, la) or not is_graph(nb, nbb, b_bonds, lb):
        return out
    a_atoms, a_bonds, b_atoms, b_bonds = a_atoms[:na], a_bonds[:nba], b_atoms[:nb], b_bonds[:nbb]
    t = Tables(a_atoms, a_bonds, b_atoms, b_bonds, mode)
    out["flags"] = PAIR
    starts = [(a0, b0) for a0 in range(na) for b0 in range(nb) if t.compat[a0] >> b0 & 1]
    if not starts:
        return out
    floor = max(Root(t, a0, b0).greedy() for a0, b0 in starts) if use_floor else (0, 0)
    out["floor"] = floor
    winner = None
    for a0, b0 in starts:
        r = Root(t, a0, b0, floor, cap).walk()
        out["roots"].append((a0, b0, r.best[0], r.best[1], r.steps, r.capped))
        out["steps"] += r.steps
        if r.capped:
            out["flags"] |= UNDECIDED
        if winner is None or r.best > winner.best:
            winner = r
    m = winner.best_map
    mask = recount(t, m)
    out["search_size"] = winner.best
    if not out["flags"] & UNDECIDED:
        assert bits(mask) == winner.best[0], (bits(mask), winner.best)
    out["size"] = (bits(mask), len(m))
    out["bond_a"] = mask
    out["flags"] |= COMMON
    new = {}
    for a in sorted(m):
        out["map_a"][a] = 1 + m[a]
        new[a] = len(new)
        out["atom_map"][a] = len(new)
        out["out_atoms"][new[a]] = a_atoms[a]
    out["out_natoms"] = len(m)
    for k, (a, b, o) in enumerate(a_bonds):
        if mask >> k & 1:
            out["out_bonds"][out["out_nbonds"]] = new[a] | new[b] << 8 | o << 16
            out["out_nbonds"] += 1
    if len(m) == na and bits(mask) == sum(1 for e in a_bonds if usable(e)):
        out["flags"] |= WHOLE_A
    image = {(m[a], m[b], o) for k, (a, b, o) in enumerate(a_bonds) if mask >> k & 1}
    if len(m) == nb and all((u, v, o) in image or (v, u, o) in image for u, v, o in b_bonds if usable((u, v, o))):
        out["flags"] |= WHOLE_B
    return out


_GRAPHS = {}


def graph_of(s):
    if s not in _GRAPHS:
        _GRAPHS[s] = K.graph(s)[2:]
    return _GRAPHS[s]


def string_mcs(a, b, mode=0, la=MAX_WIDTH, lb=MAX_WIDTH, cap=MAX_STEPS, use_floor=True):
    """Two strings; one that is no molecule has no atoms, and the pair is no pair."""
    (aa, ab), (ba, bb) = graph_of(a), graph_of(b)
    return mcs_arrays(len(aa), aa, len(ab), ab, len(ba), ba, len(bb), bb, mode, la, lb, cap, use_floor)


def similarity(out, a_atoms, a_bonds, b_atoms, b_bonds):
    """(atoms + bonds) / (A's atoms + usable entries + B's atoms + usable entries - atoms - bonds); 0 where the pair is no pair"""
    if not out["flags"] & PAIR:
        return 0.0
    common = out["size"][0] + out["size"][1]
    total = len(a_atoms) + sum(map(usable, a_bonds)) + len(b_atoms) + sum(map(usable, b_bonds))
    return common / (total - common)


def brute_force(a_atoms, a_bonds, b_atoms, b_bonds, mode=0):
    """The greatest (|E|, |M|) over every subset E of A's usable entries that is connected, every injective image of its atoms
    (compatible, every entry of E onto a B bond of its order), and every single compatible pair -> the size.  Small graphs only."""
    have = set()
    for u, v, o in b_bonds:
        if usable((u, v, o)):
            have |= {(u, v, o), (v, u, o)}
    best = (0, 1) if any(compatible(x, y, mode) for x in a_atoms for y in b_atoms) else (0, 0)
    live = [e for e in a_bonds if usable(e)]
    for size in range(1, len(live) + 1):
        for chosen in itertools.combinations(live, size):
            nodes = sorted({v for e in chosen for v in e[:2]})
            if (size, len(nodes)) <= best or len(nodes) > len(b_atoms):
                continue
            seen, grew = {nodes[0]}, True
            while grew:
                grew = False
                for a, b, _ in chosen:
                    if (a in seen) != (b in seen):
                        seen |= {a, b}
                        grew = True
            if len(seen) != len(nodes):
                continue
            for image in itertools.permutations(range(len(b_atoms)), len(nodes)):
                f = dict(zip(nodes, image))
                if all(compatible(a_atoms[a], b_atoms[f[a]], mode) for a in nodes) and \
                        all((f[a], f[b], o) in have for a, b, o in chosen):
                    best = (size, len(nodes))
                    break
    return best


def check_witness(out, a_atoms, a_bonds, b_atoms, b_bonds, mode=0):
    """Witness validity of one pair's outputs (item 2 of the host tests): raises AssertionError."""
    m = {a: v - 1 for a, v in enumerate(out["map_a"]) if v}
    if not out["flags"] & COMMON:
        assert not m and out["bond_a"] == 0 and out["size"] == (0, 0) and out["out_natoms"] == 0 and out["out_nbonds"] == 0
        return
    assert len(set(m.values())) == len(m) and all(a < len(a_atoms) and v < len(b_atoms) for a, v in m.items())
    assert all(compatible(a_atoms[a], b_atoms[v], mode) for a, v in m.items())
    have = set()
    for u, v, o in b_bonds:
        if usable((u, v, o)):
            have |= {(u, v, o), (v, u, o)}
    mask = sum(1 << k for k, (a, b, o) in enumerate(a_bonds) if usable((a, b, o)) and a in m and b in m and (m[a], m[b], o) in have)
    assert out["bond_a"] == mask and out["size"] == (bits(mask), len(m))
    seen, grew = {min(m)}, True
    while grew:
        grew = False
        for k, (a, b, _) in enumerate(a_bonds):
            if mask >> k & 1 and (a in seen) != (b in seen):
                seen |= {a, b}
                grew = True
    assert seen == set(m), (seen, m)
    new = {a: i for i, a in enumerate(sorted(m))}
    width = len(out["out_atoms"])
    assert out["out_natoms"] == len(m) and out["out_atoms"] == [a_atoms[a] for a in sorted(m)] + [0] * (width - len(m))
    kept = [new[a] | new[b] << 8 | o << 16 for k, (a, b, o) in enumerate(a_bonds) if mask >> k & 1]
    assert out["out_nbonds"] == len(kept) and out["out_bonds"] == kept + [0] * (width - len(kept))
    assert out["atom_map"] == [1 + new[a] if a in m else 0 for a in range(width)]
