"""Reference of mdt_sub_match (csrc/k_molsub.hip): the definition in include/mdt_hip.h in plain Python ints on molkey_ref.graph(),
sharing no code and no table with the package.  The depth-first search keeps the candidate word of every depth on a stack (the
kernel computes it again on the way back); the number of steps of every root is exposed, because the step cap is part of the
definition."""
import molkey_ref as K

MAX_PATTERNS, MAX_WIDTH, MAX_STEPS, MAX_TARGET = 32, 32, 4096, 64
SUBSTRUCTURE = 128
NONE, MATCH, UNDECIDED = 0, 1, 2

# the small patterns the cap was tried on before anything was built (with random_spellings(): worst root 18 steps)
PATTERNS = ["C", "N", "O", "C=O", "CC(=O)O", "c1ccccc1", "C1CC1", "C#N", "[O-]", "CCN", "c1ccncc1", "*", "C*C", "CO", "C(F)(F)F",
            "C1CCCCC1", "ccc", "C.C", "N.O", "[NH3+]", "CCCCCCCC", "C(C)(C)C", "S", "Cl", "c:c", "C-C", "C1CC1.C1CC1"]
# what every screening pipeline asks for
EVERYDAY = ["C=O", "C#N", "c1ccccc1", "C1CC1", "CC(=O)O", "N", "[O-]", "C(F)(F)F"]


def mask_of(p):
    return (0xFFFFF000 if p >> 11 & 1 else 0) | (0 if p & 31 == 26 else 0x7FF)


def accepts(p, t):
    return (p ^ t) & mask_of(p) == 0


def is_graph(n, nb, bonds, width):
    """The rule of mdt_mol_key: counts inside [1, width] x [0, width], every bond end below n."""
    return 1 <= n <= width and 0 <= nb <= width and all(a < n and b < n for a, b, _ in bonds[:nb])


def search(root, m, compat, adj, back, cap=MAX_STEPS):
    """One root -> (MATCH / NONE / UNDECIDED, steps)."""
    f, used, steps = [root] + [0] * (m - 1), 1 << root, 0

    def candidates(p):
        c = compat[p] & ~used
        for e, o in back[p]:
            c &= adj[o][f[e]]
        return c
    stack, p = [None, candidates(1)], 1
    while p >= 1:
        c = stack[p]
        if c == 0:                                                           # back
            p -= 1
            if p >= 1:
                used &= ~(1 << f[p])
            stack.pop()
            continue
        if steps == cap:
            return UNDECIDED, steps
        t = (c & -c).bit_length() - 1
        stack[p] = c & (c - 1)
        steps += 1
        f[p] = t
        if p == m - 1:
            return MATCH, steps
        used |= 1 << t
        p += 1
        stack.append(candidates(p))
    return NONE, steps


def match_arrays(n, atoms, nb, bonds, m, p_atoms, mb, p_bonds, width=MAX_TARGET, p_width=MAX_WIDTH, cap=MAX_STEPS):
    """-> (verdict, [(root, its verdict, its steps)]) for a target (n atoms, nb bonds (a, b, order)) and a pattern (m, mb); the
    counts are given apart from the lists so that arrays no scan writes can be asked about."""
    if not is_graph(n, nb, bonds, width) or not is_graph(m, mb, p_bonds, p_width) or m > n:
        return NONE, []
    bonds, p_bonds = bonds[:nb], p_bonds[:mb]
    if any(not 1 <= o <= 5 for _, _, o in p_bonds):                          # no target entry can satisfy it
        return NONE, []
    adj = [[0] * n for _ in range(6)]
    for a, b, o in bonds:
        if 1 <= o <= 5:
            adj[o][a] |= 1 << b
            adj[o][b] |= 1 << a
    back, loops = [[] for _ in range(m)], [[] for _ in range(m)]
    for a, b, o in p_bonds:
        (loops[a] if a == b else back[max(a, b)]).append((min(a, b), o))
    compat = [sum(1 << t for t in range(n) if accepts(p_atoms[p], atoms[t]) and all(adj[o][t] >> t & 1 for _, o in loops[p]))
              for p in range(m)]
    if any(c == 0 for c in compat):
        return NONE, []
    if m == 1:
        return MATCH, []
    roots = [(r,) + search(r, m, compat, adj, back, cap) for r in range(n) if compat[0] >> r & 1]
    ends = {v for _, v, _ in roots}
    return (MATCH if MATCH in ends else UNDECIDED if UNDECIDED in ends else NONE), roots


_GRAPHS = {}


def graph_of(s):
    if s not in _GRAPHS:
        _GRAPHS[s] = K.graph(s)[2:]
    return _GRAPHS[s]


def string_match(pattern, target, cap=MAX_STEPS):
    """-> (verdict, the largest step count of a root) for two strings; one that is no molecule has no atoms."""
    (pa, pb), (ta, tb) = graph_of(pattern), graph_of(target)
    verdict, roots = match_arrays(len(ta), ta, len(tb), tb, len(pa), pa, len(pb), pb, cap=cap)
    return verdict, max([s for _, _, s in roots], default=0)


def contains(pattern, target):
    verdict, _ = string_match(pattern, target)
    assert verdict != UNDECIDED, (pattern, target)
    return verdict == MATCH


def words(targets, patterns):
    """-> ([match word], [undecided word]) per target string, bit q for pattern q."""
    match, undecided = [], []
    for t in targets:
        verdicts = [string_match(p, t)[0] for p in patterns]
        match.append(sum(1 << q for q, v in enumerate(verdicts) if v == MATCH))
        undecided.append(sum(1 << q for q, v in enumerate(verdicts) if v == UNDECIDED))
    return match, undecided


def flag(match, undecided, need, ban):
    return SUBSTRUCTURE if (match & need) != need or ((match | undecided) & ban) != 0 else 0
