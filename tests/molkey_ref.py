"""String-level reference of mdt_mol_graph / mdt_mol_key (csrc/k_molgraph.hip): plain Python and numpy written from the definition in
include/mdt_hip.h, sharing no code and no table with the package.  graph(s) -> (status, position, descriptors, bonds) reuses
smiles_ref's rules for status and position; key(descriptors, bonds) is the rooted refinement hash.

Also a generator of random molecular graphs and a writer of random spellings of a graph, for the invariance tests."""
import random

import numpy as np

import smiles_ref as S

MASK = (1 << 64) - 1
ROOT, K = 0xA5A5A5A5A5A5A5A5, 0x100000001B3
SYMBOL_ORDER = {"-": 1, "/": 1, "\\": 1, "=": 2, "#": 3, "$": 4, ":": 5}
ORDER_SYMBOL = {1: "-", 2: "=", 3: "#", 4: "$", 5: ":"}
MAX_TOKENS = 64

# the pairs the definition was agreed on: two spellings of one molecule; two molecules
EQUAL_PAIRS = [("CCO", "OCC"), ("C1CC1C", "CC1CC1"), ("C=CC", "CC=C"), ("C1CCCCC1", "C%12CCCCC%12"), ("C1=CC=CC=C1", "C=1C=CC=CC1"),
               ("F/C=C/F", "F/C=C\\F")]
DIFFERENT_PAIRS = [("CCO", "COC"), ("CC(C)C", "CCCC"), ("C1CCCCC1", "CCCCCC"), ("C1CC1.C1CC1", "C1CCCCC1"),
                   ("C12C3C4C1C5C2C3C45", "C12C3C1C1C4C2C3C41"), ("C1CCC2CCCCC2C1", "C1CCCC1C1CCCC1"), ("CC=O", "C=CO"),
                   ("C[NH3+]", "CN"), ("c1ccccc1", "C1=CC=CC=C1")]


def descriptor(symbol, bracket=False, charge=0, hcount=0, isotope=0):
    """The 32-bit atom descriptor (include/mdt_hip.h, mdt_mol_graph).  symbol: 'C', 'Cl', 'c', '*', ..."""
    first = 26 if symbol == "*" else ord(symbol[0].upper()) - 65
    second = 1 + ord(symbol[1]) - 97 if len(symbol) == 2 else 0
    aromatic = symbol[0].islower()
    return (first | second << 5 | int(aromatic) << 10 | int(bracket) << 11 | (charge + 9) << 12 | hcount << 17 |
            (isotope % 2048) << 21)


def bracket_descriptor(body):
    """body: what stands between '[' and ']' of a bracket atom that smiles_ref accepts."""
    k = 0
    while body[k] in S.DIGITS:
        k += 1
    isotope = int(body[:k]) if k else 0
    if body[k] in S.UPPER and body[k:k + 2] in S.ELEMENTS and body[k + 1:k + 2] in S.LOWER:
        symbol = body[k:k + 2]
    else:
        symbol = body[k]
    k += len(symbol)
    rest = body[k:].lstrip("@")
    hcount = charge = 0
    if rest[:1] == "H":
        hcount, rest = 1, rest[1:]
        if rest[:1] in S.DIGITS and rest[:1]:
            hcount, rest = int(rest[0]), rest[1:]
    if rest[:1] in ("+", "-"):
        sign, rest = rest[0], rest[1:]
        charge = 1
        if rest[:1] == sign:
            charge, rest = 2, rest[1:]
        elif rest[:1] in S.DIGITS and rest[:1]:
            charge, rest = int(rest[0]), rest[1:]
        if sign == "-":
            charge = -charge
    assert rest == "" or rest[0] == ":", (body, rest)                        # the atom class is ignored
    return descriptor(symbol, True, charge, hcount, isotope)


def graph(s):
    """-> (status, position, descriptors, bonds): smiles_ref's verdict, and for an OK row the atoms in order of appearance and the
    bonds (a, b, order) in order of creation.  Anything else has no atoms and no bonds."""
    status, position = S.check(s)
    if status != S.OK:
        return status, position, [], []
    atoms, aromatic, bonds = [], [], []
    current, parents, pending, rings, fresh = None, [], None, {}, True      # fresh: at the start or after a dot

    def join(a, b, symbol):
        order = SYMBOL_ORDER[symbol] if symbol else (5 if aromatic[a] and aromatic[b] else 1)
        bonds.append((a, b, order))
    j, n = 0, len(s)
    while j < n:
        ch = s[j]
        atom = None
        if ch == "[":
            end = S.bracket_atom(s, j)
            atom, j = bracket_descriptor(s[j + 1:end - 1]), end
        elif s[j:j + 2] in ("Cl", "Br"):
            atom, j = descriptor(s[j:j + 2]), j + 2
        elif ch in S.ORGANIC or ch in S.AROMATIC or ch == "*":
            atom, j = descriptor(ch), j + 1
        if atom is not None:
            atoms.append(atom)
            aromatic.append(bool(atom >> 10 & 1))
            if not fresh:
                join(current, len(atoms) - 1, pending)
            current, pending, fresh = len(atoms) - 1, None, False
        elif ch in SYMBOL_ORDER:
            pending, j = ch, j + 1
        elif ch in S.DIGITS or ch == "%":
            number, j = (int(s[j + 1:j + 3]), j + 3) if ch == "%" else (int(ch), j + 1)
            if number in rings:
                opener, symbol = rings.pop(number)
                join(opener, current, symbol or pending)
            else:
                rings[number] = (current, pending)
            pending = None
        elif ch == "(":
            parents.append(current)
            j += 1
        elif ch == ")":
            current = parents.pop()
            j += 1
        else:
            assert ch == ".", (s, j)
            fresh, j = True, j + 1
    return status, position, atoms, bonds


def mix(x):
    """One splitmix64 step on a Python int or a numpy uint64 array."""
    if isinstance(x, np.ndarray):
        with np.errstate(over="ignore"):
            z = x + np.uint64(0x9E3779B97F4A7C15)
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            return z ^ (z >> np.uint64(31))
    z = (x + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def key(descriptors, bonds, rooted=True):
    """The 64-bit graph key as a Python int; 0 for no atoms.  Columns of ``lab`` are the roots.  rooted=False: the plain form of the
    same hash (one labelling, no root), which the tests show to be too weak."""
    n = len(descriptors)
    if n == 0:
        return 0
    seed = mix(np.array(descriptors, dtype=np.uint64))
    roots = n if rooted else 1
    lab = np.tile(seed[:, None], (1, roots))
    if rooted:
        lab[np.arange(n), np.arange(n)] = mix(seed ^ np.uint64(ROOT))
    ends = np.array([(a, b) for a, b, _ in bonds], dtype=np.int64).reshape(-1, 2)
    ok = np.array([order * K & MASK for _, _, order in bonds], dtype=np.uint64)[:, None]
    with np.errstate(over="ignore"):
        for _ in range(n):
            acc = np.zeros((n, roots), dtype=np.uint64)
            np.add.at(acc, ends[:, 0], mix(lab[ends[:, 1]] + ok))            # (add.at: an atom may occur in many bonds)
            np.add.at(acc, ends[:, 1], mix(lab[ends[:, 0]] + ok))
            lab = mix(lab ^ mix(acc))
        h = mix(lab).sum(axis=0, dtype=np.uint64)
        total = int(mix(h).sum(dtype=np.uint64))
    return mix((total + n + (len(bonds) << 32)) & MASK) or 1


_KEYS = {}


def string_key(s):
    """The key of a string (0 unless it is an OK, non-empty row); each distinct string is computed once."""
    if s not in _KEYS:
        _, _, atoms, bonds = graph(s)
        _KEYS[s] = key(atoms, bonds)
    return _KEYS[s]


# ----------------------------------------------------------------------------------------------------------------------
# random graphs and random spellings
# ----------------------------------------------------------------------------------------------------------------------
# (how the atom is written, free valences it is given here); bracket atoms are exempt from the check, the budget keeps them sane
PLAIN = [("C", 4)] * 8 + [("N", 3)] * 3 + [("O", 2)] * 3 + [("S", 2), ("F", 1), ("Cl", 1), ("Br", 1), ("P", 3), ("B", 3), ("*", 2)]
BRACKET = [("[O-]", 1), ("[N+]", 4), ("[13CH3]", 1), ("[NH3+]", 1), ("[C@H]", 3), ("[Si]", 4), ("[nH]", 0), ("[2H]", 1), ("[Fe+2]", 2)]
LONE = ["[NH4+]", "[Na+]", "[Cl-]", "[OH-]", "[Ca+2]", "O", "C"]
AROMATIC_RINGS = ["cccccc", "ccccnc", "ccncnc", "cccco", "cccs[nH]", "cc[nH]cn"]


class Graph:
    """atoms: how each atom is written; bonds: (a, b, order), a simple graph (no pair bonded twice, no self bond)."""

    def __init__(self, atoms, bonds):
        self.atoms, self.bonds = atoms, bonds

    def aromatic(self, a):
        return self.atoms[a].lstrip("[0123456789")[0].islower()

    def descriptors(self):
        return [bracket_descriptor(t[1:-1]) if t[0] == "[" else descriptor(t) for t in self.atoms]

    def components(self):
        comp = list(range(len(self.atoms)))

        def find(a):
            while comp[a] != a:
                a = comp[a]
            return a
        for a, b, _ in self.bonds:
            comp[find(a)] = find(b)
        groups = {}
        for a in range(len(self.atoms)):
            groups.setdefault(find(a), []).append(a)
        return list(groups.values())


def random_graph(rng, max_atoms=20):
    """Trees plus 0 to 3 ring bonds within the valences, now and then grown from an aromatic ring, with bracket atoms and up to
    three dotted components."""
    atoms, free, bonds = [], [], []
    budget = max(rng.randint(1, max_atoms), rng.randint(1, max_atoms))
    for _ in range(rng.choice([1, 1, 1, 1, 2, 2, 3])):
        if len(atoms) >= budget:
            break
        first = len(atoms)
        if rng.random() < 0.15:                                              # a counter-ion or a lone small molecule
            atoms.append(rng.choice(LONE))
            free.append(0)
            continue
        if rng.random() < 0.3 and budget - len(atoms) >= 6:                   # an aromatic ring to grow from
            ring = rng.choice(AROMATIC_RINGS)
            names = ["[nH]" if t == "[" else t for t in ring.replace("[nH]", "[")]
            for i, t in enumerate(names):
                atoms.append(t)
                free.append(1 if t == "c" else 0)
            m = len(names)
            bonds += [(first + i, first + (i + 1) % m, 5) for i in range(m)]
        else:
            t, v = rng.choice(PLAIN if rng.random() < 0.85 else BRACKET)
            atoms.append(t)
            free.append(v)
        size = rng.randint(0, budget - len(atoms))
        for _ in range(size):                                                # the tree
            open_ = [a for a in range(first, len(atoms)) if free[a] > 0]
            if not open_:
                break
            a = rng.choice(open_)
            t, v = rng.choice(PLAIN if rng.random() < 0.85 else BRACKET)
            if v == 0:
                continue
            aromatic_a = atoms[a] == "c"
            order = 1 if aromatic_a else rng.choice([o for o in (1, 1, 1, 1, 2, 2, 3, 4) if o <= min(free[a], v)])
            atoms.append(t)
            free.append(v - order)
            free[a] -= order
            bonds.append((a, len(atoms) - 1, order))
        for _ in range(rng.randint(0, 3)):                                   # ring bonds
            open_ = [a for a in range(first, len(atoms)) if free[a] > 0 and atoms[a] != "c"]
            if len(open_) < 2:
                break
            a, b = rng.sample(open_, 2)
            if any({a, b} == {x, y} for x, y, _ in bonds):
                continue
            order = rng.choice([o for o in (1, 1, 1, 2) if o <= min(free[a], free[b])])
            free[a] -= order
            free[b] -= order
            bonds.append((a, b, order))
    return Graph(atoms, bonds)


def spell(g, rng):
    """One random spelling: start atoms, neighbour order, ring numbers (with %nn), the end of a closure that carries the bond symbol,
    optional explicit symbols where the default would do, and the order of the components all vary."""
    nbrs = {a: [] for a in range(len(g.atoms))}
    for e, (a, b, order) in enumerate(g.bonds):
        nbrs[a].append((b, e))
        nbrs[b].append((a, e))
    for a in nbrs:
        rng.shuffle(nbrs[a])

    def symbol(e, must_not_skip=False):
        a, b, order = g.bonds[e]
        default = 5 if g.aromatic(a) and g.aromatic(b) else 1
        if order == default and not must_not_skip and rng.random() < 0.85:
            return ""
        return ORDER_SYMBOL[order]

    def needs_symbol(e):
        a, b, order = g.bonds[e]
        return order != (5 if g.aromatic(a) and g.aromatic(b) else 1)
    pieces = []
    comps = g.components()
    rng.shuffle(comps)
    for comp in comps:
        start = rng.choice(comp)
        # pass 1: which bonds are tree bonds, which close rings (seen from the later atom towards an earlier one)
        seen, tree, closures = set(), set(), {a: [] for a in comp}
        done = set()

        def explore(a):
            seen.add(a)
            for b, e in nbrs[a]:
                if e in done:
                    continue
                done.add(e)
                if b in seen:
                    closures[a].append(e)
                    closures[b].append(e)
                else:
                    tree.add(e)
                    explore(b)
        explore(start)
        # pass 2: write
        out, opened, in_use = [], {}, set()

        def digits(number):
            return "%%%02d" % number if number >= 10 or rng.random() < 0.2 else str(number)

        def write(a, via):
            out.append(g.atoms[a])
            mine = list(closures[a])
            rng.shuffle(mine)
            for e in mine:
                if e not in opened:                                          # this end comes first in the string: it opens
                    number = rng.choice([k for k in (list(range(1, 10)) * 8 + list(range(0, 100))) if k not in in_use])
                    in_use.add(number)
                    where = rng.choice(["open", "close", "both"]) if needs_symbol(e) else rng.choice(["open", "close", "none", "none"])
                    opened[e] = (number, where)
                    out.append((ORDER_SYMBOL[g.bonds[e][2]] if where in ("open", "both") else "") + digits(number))
                else:
                    number, where = opened[e]
                    in_use.discard(number)
                    out.append((ORDER_SYMBOL[g.bonds[e][2]] if where in ("close", "both") else "") + digits(number))
            children = [(b, e) for b, e in nbrs[a] if e in tree and e != via and b not in written]
            for i, (b, e) in enumerate(children):
                if b in written:
                    continue
                last = i == len(children) - 1
                if not last:
                    out.append("(")
                out.append(symbol(e))
                written.add(b)
                write(b, e)
                if not last:
                    out.append(")")
        written = {start}
        write(start, None)
        pieces.append("".join(out))
    return ".".join(pieces)


def random_spellings(graphs=500, spellings=4, seed=5, max_atoms=20):
    """-> list of (Graph, [spellings]): every spelling passes smiles_ref.check and has at most 64 tokens (graphs that do not fit
    are redrawn).  Deterministic."""
    rng = random.Random(seed)
    out = []
    while len(out) < graphs:
        g = random_graph(rng, max_atoms)
        written = [spell(g, rng) for _ in range(spellings)]
        if max(len(s) for s in written) > MAX_TOKENS:
            continue
        out.append((g, written))
    return out
