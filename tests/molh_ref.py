"""Reference of mdt_mol_hydrogens (csrc/k_molh.hip): the definition in include/mdt_hip.h in plain Python ints on molkey_ref.graph(),
sharing no code and no table with the package.  Per atom the hydrogens it carries and whether it still wants a double bond; per row
whether those double bonds can be placed (a perfect matching of the wanting atoms over the aromatic bonds), found by the search
whose order -- and therefore whose step count -- is part of the definition; and the molecular formula."""
import molkey_ref as K

MAX_STEPS, MAX_WIDTH = 4096, 64
OK, AROMATIC_OVERVALENT, NO_KEKULE, UNDECIDED = 0, 1, 2, 3
OVERVALENT_BIT = 64
SLOTS = ("H", "B", "C", "N", "O", "F", "P", "S", "Cl", "Br", "I", "other", "charge")
VALENCES = {"B": (3,), "C": (4,), "N": (3, 5), "O": (2,), "P": (3, 5), "S": (2, 4, 6), "F": (1,), "Cl": (1,), "Br": (1,), "I": (1,)}
AROMATIC = "BCNOPS"
GROUP = {"B": 13, "C": 14, "N": 15, "O": 16, "P": 15, "S": 16}
GROUP_VALENCES = {13: (3,), 14: (4,), 15: (3, 5), 16: (2, 4, 6)}
WEIGHTS = {"H": 1.008, "B": 10.81, "C": 12.011, "N": 14.007, "O": 15.999, "F": 18.998403163, "P": 30.973761998, "S": 32.06,
           "Cl": 35.45, "Br": 79.904, "I": 126.90447}


def fields(d):
    """descriptor -> (symbol in upper-case-first form or '*', aromatic, bracket, charge, bracket H count)"""
    first, second = d & 31, d >> 5 & 31
    symbol = "*" if first == 26 else chr(65 + first) + (chr(96 + second) if second else "")
    return symbol, bool(d >> 10 & 1), bool(d >> 11 & 1), (d >> 12 & 31) - 9, d >> 17 & 15


def at_least(valences, s):
    return min([v for v in valences if v >= s], default=None)


def atom_rule(d, sum1):
    """-> (hydrogens, wants a double bond, aromatic-overvalent)"""
    symbol, aromatic, bracket, charge, hcount = fields(d)
    if bracket:
        if not aromatic or symbol not in GROUP:
            return hcount, False, False
        v = at_least(GROUP_VALENCES.get(GROUP[symbol] - charge, ()), sum1 + hcount)
        return hcount, v is not None and v - (sum1 + hcount) >= 1, False
    if aromatic:
        v = at_least(VALENCES[symbol], sum1) if symbol in AROMATIC else None
        if v is None:
            return 0, False, True
        wants = v - sum1 >= 1
        return v - sum1 - int(wants), wants, False
    v = at_least(VALENCES.get(symbol, ()), sum1)
    return (0 if v is None else v - sum1), False, False


def search(wanting, adj, cap):
    """The matching of the definition -> (verdict, steps, {atom: partner}).  adj[a]: the set of atoms joined to a by an edge."""
    unmatched, steps, frames = set(wanting), 0, []
    if not unmatched:
        return OK, 0, {}

    def open_frame():
        u = min(unmatched, key=lambda a: (len(adj[a] & unmatched), a))
        frames.append([u, sorted(adj[u] & unmatched), None])
    open_frame()
    while True:
        u, candidates, v = frames[-1]
        if v is not None:                                                    # back: the pair is restored
            unmatched |= {u, v}
            frames[-1][2] = None
        if not candidates:
            frames.pop()
            if not frames:
                return NO_KEKULE, steps, {}
            continue
        if steps == cap:
            return UNDECIDED, steps, {}
        v = candidates.pop(0)
        steps += 1
        frames[-1][2] = v
        unmatched -= {u, v}
        if not unmatched:
            pairs = {}
            for a, _, b in frames:
                pairs[a], pairs[b] = b, a
            return OK, steps, pairs
        open_frame()


def is_graph(n, nb, bonds, width):
    return 1 <= n <= width and 0 <= nb <= width and all(a < n and b < n for a, b, _ in bonds[:nb])


def hydrogens_arrays(n, atoms, nb, bonds, width=MAX_WIDTH, cap=MAX_STEPS):
    """-> dict(verdict, atom, hydrogens [width], partner [width], formula [13], steps, wanting) for a row of n atoms and nb bonds
    (a, b, order); the counts are given apart from the lists so that arrays no scan writes can be asked about."""
    out = dict(verdict=OK, atom=-1, hydrogens=[0] * width, partner=[0] * width, formula=[0] * 13, steps=0, wanting=[], edges=[])
    if not is_graph(n, nb, bonds, width):
        return out
    atoms, bonds = atoms[:n], bonds[:nb]
    sum1 = [0] * n
    for a, b, o in bonds:
        sum1[a] += 1 if o == 5 else o
        sum1[b] += 1 if o == 5 else o
    rules = [atom_rule(d, s) for d, s in zip(atoms, sum1)]
    wanting = [a for a, (_, w, _) in enumerate(rules) if w]
    adj = {a: set() for a in wanting}
    for a, b, o in bonds:
        if o == 5 and a != b and a in adj and b in adj:
            adj[a].add(b)
            adj[b].add(a)
    over = [a for a, (_, _, x) in enumerate(rules) if x]
    out["wanting"], out["edges"] = wanting, sorted({(min(a, b), max(a, b)) for a in adj for b in adj[a]})
    for a, (h, _, _) in enumerate(rules):
        out["hydrogens"][a] = h
    formula = out["formula"]
    for d, (h, _, _) in zip(atoms, rules):
        symbol, _, _, charge, _ = fields(d)
        formula[0] += h
        formula[SLOTS.index(symbol) if symbol in SLOTS[:11] else 11] += 1
        formula[12] += charge
    if over:
        out["verdict"], out["atom"] = AROMATIC_OVERVALENT, over[0]
    elif len(wanting) % 2:
        out["verdict"] = NO_KEKULE
    else:
        out["verdict"], out["steps"], pairs = search(wanting, adj, cap)
        for a, b in pairs.items():
            out["partner"][a] = 1 + b
    return out


_ROWS = {}


def string_hydrogens(s, cap=MAX_STEPS, width=MAX_WIDTH):
    """The answer for a string; one that is no molecule has no atoms."""
    at = (s, cap, width)
    if at not in _ROWS:
        _, _, atoms, bonds = K.graph(s)
        _ROWS[at] = hydrogens_arrays(len(atoms), atoms, len(bonds), bonds, width, cap)
    return _ROWS[at]


def formula_string(counts):
    """Hill order: C, H, then the rest by symbol; without carbon all by symbol; the charge as + / - / +2 / -2; '?' at the end when an
    atom is none of the eleven; '' for no atoms."""
    count = dict(zip(SLOTS, counts))
    if not any(counts[:12]):
        return ""
    order = ["C", "H"] + sorted(s for s in SLOTS[:11] if s not in "CH") if count["C"] else sorted(SLOTS[:11])
    text = "".join(s + (str(count[s]) if count[s] > 1 else "") for s in order if count[s])
    q = count["charge"]
    text += ("+" if q > 0 else "-") + (str(abs(q)) if abs(q) > 1 else "") if q else ""
    return text + ("?" if count["other"] else "")


def weight(counts):
    if counts[11]:
        return float("nan")
    return sum(WEIGHTS[s] * c for s, c in zip(SLOTS[:11], counts))
