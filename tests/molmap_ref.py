"""Reference of mdt_sub_map (csrc/k_molsub.hip, k_sub_map): the definition in include/mdt_hip.h in plain Python ints on
molkey_ref.graph(), sharing no code and no table with the package.  Two things: the ENUMERATION (molsub_ref's depth-first search run
to the end of every root's tree, under its step cap), and an INDEPENDENT checker that knows nothing of the search --
itertools.permutations over all injective maps, each tested with the atom rule and the bond rule alone."""
import itertools

import molsub_ref as B

SUBSTRUCTURE = B.SUBSTRUCTURE


def enumerate_root(root, m, compat, adj, back, cap=B.MAX_STEPS):
    """One root to the end of its tree -> (embeddings seen, capped, steps, the union of their images, the first map or None)."""
    f, used, steps, seen, cover, first = [root] + [0] * (m - 1), 1 << root, 0, 0, 0, None

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
            return seen, True, steps, cover, first
        t = (c & -c).bit_length() - 1
        stack[p] = c & (c - 1)
        steps += 1
        f[p] = t
        if p == m - 1:                                                       # a full map: counted, and on at the same depth
            seen += 1
            cover |= used | 1 << t
            first = first or list(f)
            continue
        used |= 1 << t
        p += 1
        stack.append(candidates(p))
    return seen, False, steps, cover, first


def tables(n, atoms, nb, bonds, m, p_atoms, mb, p_bonds, width, p_width):
    """What is decided before any search -> None (no match), or (compat, adj, back)"""
    if not B.is_graph(n, nb, bonds, width) or not B.is_graph(m, mb, p_bonds, p_width) or m > n:
        return None
    bonds, p_bonds = bonds[:nb], p_bonds[:mb]
    if any(not 1 <= o <= 5 for _, _, o in p_bonds):
        return None
    adj = [[0] * n for _ in range(6)]
    for a, b, o in bonds:
        if 1 <= o <= 5:
            adj[o][a] |= 1 << b
            adj[o][b] |= 1 << a
    back, loops = [[] for _ in range(m)], [[] for _ in range(m)]
    for a, b, o in p_bonds:
        (loops[a] if a == b else back[max(a, b)]).append((min(a, b), o))
    compat = [sum(1 << t for t in range(n) if B.accepts(p_atoms[p], atoms[t]) and all(adj[o][t] >> t & 1 for _, o in loops[p]))
              for p in range(m)]
    if any(c == 0 for c in compat):
        return None
    return compat, adj, back


def map_arrays(n, atoms, nb, bonds, m, p_atoms, mb, p_bonds, width=B.MAX_TARGET, p_width=B.MAX_WIDTH, cap=B.MAX_STEPS):
    """-> dict(found, capped, embeddings, cover: ints; map: p_width bytes, 1 + f(p); roots: [(root, seen, capped, steps)])"""
    out = dict(found=0, capped=0, embeddings=0, cover=0, map=[0] * p_width, roots=[])
    made = tables(n, atoms, nb, bonds, m, p_atoms, mb, p_bonds, width, p_width)
    if made is None:
        return out
    compat, adj, back = made
    if m == 1:
        lowest = (compat[0] & -compat[0]).bit_length() - 1
        out.update(found=compat[0], cover=compat[0], embeddings=bin(compat[0]).count("1"), map=[1 + lowest] + [0] * (p_width - 1))
        return out
    first = None
    for r in range(n):
        if not compat[0] >> r & 1:
            continue
        seen, capped, steps, cover, its_first = enumerate_root(r, m, compat, adj, back, cap)
        out["roots"].append((r, seen, capped, steps))
        out["found"] |= (seen > 0) << r
        out["capped"] |= capped << r
        out["embeddings"] += seen
        out["cover"] |= cover
        first = first or its_first
    if first:
        out["map"] = [1 + t for t in first] + [0] * (p_width - m)
    return out


def string_map(pattern, target, width=B.MAX_TARGET, p_width=B.MAX_WIDTH, cap=B.MAX_STEPS):
    (pa, pb), (ta, tb) = B.graph_of(pattern), B.graph_of(target)
    return map_arrays(len(ta), ta, len(tb), tb, len(pa), pa, len(pb), pb, width, p_width, cap)


def brute_force(n, atoms, nb, bonds, m, p_atoms, mb, p_bonds):
    """Every injective map of the pattern's atoms into the target's, tested with the two rules alone -> the sorted list of valid
    maps (tuples f).  Knows nothing of compat words, back-bonds, roots or steps; graphs that are molecules only."""
    have = set()
    for a, b, o in bonds[:nb]:
        have |= {(a, b, o), (b, a, o)}
    return [f for f in itertools.permutations(range(n), m)
            if all(B.accepts(p_atoms[p], atoms[f[p]]) for p in range(m)) and all((f[a], f[b], o) in have for a, b, o in p_bonds[:mb])]


def count_flag(found, capped, lo, hi):
    """The flag of one row from its per-pattern words and bounds."""
    for fnd, cap, low, high in zip(found, capped, lo, hi):
        c, u = bin(fnd).count("1"), bin(cap & ~fnd).count("1")
        if not (low <= c and c + u <= high):
            return SUBSTRUCTURE
    return 0
