"""Reference of mdt_mol_canon (csrc/k_molcanon.hip): the definition in include/mdt_hip.h in plain Python ints and lists on
molkey_ref.graph() arrays, sharing only molkey_ref's parser, mix and constants.  canon() is the search -- refinement with marks, the
twin classes, the target class, the leaf certificates, the smallest of them per component, the components in ascending
(certificate, lowest index), the node cap; brute() is an independent canoniser for rows of at most 7 atoms: the smallest certificate
over ALL numberings of a component, no refinement and no search tree in it."""
import itertools

import numpy as np

import molkey_ref as K

MAX_WIDTH, MAX_NODES = 64, 4096
CANONICAL, UNDECIDED = 1, 2                                                  # the flags; 0: no molecule


def is_graph(n, nb, bonds, width):
    return 1 <= n <= width and 0 <= nb <= width and all(a < n and b < n for a, b, _ in bonds[:nb])


def refine_many(atoms, bonds, mark_lists):
    """The labels after n rounds from the labellings that mark each list of `mark_lists` in its order -> [k] lists of n ints
    (numpy columns, one per list: the arithmetic of molkey_ref.key)"""
    n, k = len(atoms), len(mark_lists)
    seed = K.mix(np.array(atoms, dtype=np.uint64))
    lab = np.tile(seed[:, None], (1, k))
    for col, marks in enumerate(mark_lists):
        for j, m in enumerate(marks):
            lab[m, col] = K.mix(int(seed[m]) ^ ((K.ROOT + j) & K.MASK))
    with np.errstate(over="ignore"):
        if bonds:                                                            # every entry twice, sorted by the atom that takes the term
            takes = np.array([a for a, _, _ in bonds] + [b for _, b, _ in bonds], dtype=np.int64)
            gives = np.array([b for _, b, _ in bonds] + [a for a, _, _ in bonds], dtype=np.int64)
            ok = np.array([o * K.K & K.MASK for _, _, o in bonds] * 2, dtype=np.uint64)[:, None]
            by = np.argsort(takes, kind="stable")
            takes, gives, ok = takes[by], gives[by], ok[by]
            named, starts = np.unique(takes, return_index=True)
        for _ in range(n):
            acc = np.zeros((n, k), dtype=np.uint64)
            if bonds:
                acc[named] = np.add.reduceat(K.mix(lab[gives] + ok), starts, axis=0)
            lab = K.mix(lab ^ K.mix(acc))
    return [[int(x) for x in lab[:, col]] for col in range(k)]


def refine(atoms, bonds, marks):
    return refine_many(atoms, bonds, [marks])[0]


def components(n, bonds):
    """-> the components (sorted lists) of the graph of the pairs a != b named by an entry, by lowest atom"""
    comp = list(range(n))
    changed = True
    while changed:
        changed = False
        for a, b, _ in bonds:
            low = min(comp[a], comp[b])
            if comp[a] != low or comp[b] != low:
                comp[a] = comp[b] = low
                changed = True
    return [[a for a in range(n) if comp[a] == c] for c in sorted(set(comp))]


def twin_keys(atoms, bonds):
    """-> per atom None, or what twins share: (the other atom, the order, the atom word) of the ONE entry that names it.  An entry
    (a, a) names a twice."""
    ends = [[] for _ in atoms]
    for a, b, o in bonds:
        ends[a].append((b, o))
        ends[b].append((a, o))
    return [(e[0][0], e[0][1], atoms[a]) if len(e) == 1 else None for a, e in enumerate(ends)]


def target(members, marks, lab, twin):
    """The class of unmarked atoms of the component with the smallest label among those of at least 2 atoms that are not twin
    classes -> sorted list, or [] for a leaf"""
    classes = {}
    for a in members:
        if a not in marks:
            classes.setdefault(lab[a], []).append(a)
    best = None
    for label, cls in classes.items():
        if len(cls) < 2 or (twin[cls[0]] is not None and all(twin[a] == twin[cls[0]] for a in cls)):
            continue
        if best is None or label < best:
            best = label
    return [] if best is None else classes[best]


def certificate(members, atoms, bonds, order):
    """order: the atoms of the component, position after position -> the certificate as a tuple of ints"""
    pos = {a: p for p, a in enumerate(order)}
    inside = sorted((min(pos[a], pos[b]), max(pos[a], pos[b]), o) for a, b, o in bonds if a in pos)
    return (len(members),) + tuple(atoms[a] for a in order) + (len(inside),) + tuple(x for e in inside for x in e)


class Undecided(Exception):
    pass


def search(members, atoms, bonds, twin, budget):
    """One component -> (the smallest certificate, the order that gives it, leaves, nodes); raises Undecided past `budget` nodes"""
    best, count = [None, None], [0, 0]                                       # (certificate, order), (leaves, nodes)

    def node(marks, lab):
        count[1] += 1
        if count[1] > budget:
            raise Undecided
        cls = target(members, marks, lab, twin)
        if not cls:
            count[0] += 1
            order = sorted(members, key=lambda a: (lab[a], a))
            cert = certificate(members, atoms, bonds, order)
            key = (cert, sorted(range(len(order)), key=lambda p: order[p]))       # ... then the positions in ascending atom index
            if best[0] is None or key < (best[0], sorted(range(len(order)), key=lambda p: best[1][p])):
                best[:] = [cert, order]
            return
        for a, child in zip(cls, refine_many(atoms, bonds, [marks + [a] for a in cls])):
            node(marks + [a], child)
    node([], refine(atoms, bonds, []))
    return best[0], best[1], count[0], count[1]


def canon(n, atoms, nb, bonds, width=MAX_WIDTH, max_nodes=MAX_NODES):
    """mdt_mol_canon of one row -> dict(priority [width], canon_atoms [width], canon_bonds [width] (words), flags, nodes, leaves)"""
    out = dict(priority=[0] * width, canon_atoms=[0] * width, canon_bonds=[0] * width, flags=0, nodes=0, leaves=0)
    if not is_graph(n, nb, bonds, width):
        return out
    atoms, bonds = list(atoms[:n]), list(bonds[:nb])
    twin = twin_keys(atoms, bonds)
    found, nodes, leaves = [], 0, 0
    for members in components(n, bonds):
        try:
            cert, order, lv, nd = search(members, atoms, bonds, twin, max_nodes - nodes)
        except Undecided:
            out.update(flags=UNDECIDED, nodes=max_nodes + 1)
            return out
        nodes, leaves = nodes + nd, leaves + lv
        found.append((cert, members[0], order))
    found.sort()
    offset, words = 0, []
    for cert, _, order in found:
        for p, a in enumerate(order):
            out["priority"][a] = 1 + offset + p
            out["canon_atoms"][offset + p] = atoms[a]
        size, inside = cert[0], cert[cert[0] + 2:]
        words += [(inside[k] + offset) | (inside[k + 1] + offset) << 8 | inside[k + 2] << 16 for k in range(0, len(inside), 3)]
        offset += size
    out["canon_bonds"][:len(words)] = words
    out.update(flags=CANONICAL, nodes=nodes, leaves=leaves)
    return out


_ROWS = {}


def string_canon(s, width=MAX_WIDTH):
    """canon() of the graph of a string as mdt_mol_graph reads it (no molecule for a row of status != 0)"""
    if (s, width) not in _ROWS:
        _, _, atoms, bonds = K.graph(s)
        _ROWS[s, width] = canon(len(atoms), atoms, len(bonds), bonds, width)
    return _ROWS[s, width]


def form(out):
    """What two rows of one graph share: the relabelled arrays"""
    return tuple(out["canon_atoms"]), tuple(out["canon_bonds"])


def brute(atoms, bonds):
    """The canonical form by brute force (n <= 7): per component the smallest certificate over all its numberings, the components
    in ascending certificate -> a tuple of certificates"""
    assert len(atoms) <= 7
    certs = []
    for members in components(len(atoms), bonds):
        certs.append(min(certificate(members, atoms, bonds, list(order)) for order in itertools.permutations(members)))
    return tuple(sorted(certs))


def edge_rows():
    """Graph arrays handed in as they are -> list of (width, n, nb, atoms, bonds)"""
    c, f = K.descriptor("C"), K.descriptor("F")
    return [
        (8, 1, 0, [c], []),                                                                        # n = 1
        (64, 64, 63, [c] * 64, [(i, i + 1, 1) for i in range(63)]),                                # the 64-atom chain
        (64, 64, 64, [c] * 64, [(i, (i + 1) % 64, 1) for i in range(64)]),                         # the 64-membered ring
        (8, 5, 4, [c, f, f, f, f], [(0, k, 1) for k in range(1, 5)]),                              # CF4
        (8, 3, 3, [c] * 3, [(0, 1, 1), (1, 1, 1), (1, 2, 1)]),                                     # an entry (a, a)
        (8, 4, 5, [c] * 4, [(0, 1, 1), (1, 2, 1), (2, 1, 2), (2, 3, 1), (3, 0, 1)]),              # a pair named twice
        (8, 4, 0, [c, f, c, f], []),                                                               # nbonds = 0
        (8, 0, 0, [], []), (8, 9, 0, [c] * 9, []), (8, 3, 9, [c] * 3, [(0, 1, 1)] * 9),            # counts out of range
        (8, 3, 2, [c] * 3, [(0, 1, 1), (1, 3, 1)]),                                                # an end beyond n
    ]


def write_priority(n, atoms, nb, bonds, width=MAX_WIDTH):
    """The priority of the canonical=True spellings: the search's where the row is decided, mdt_mol_rank's where it is not"""
    import molwrite_ref as W
    out = canon(n, atoms, nb, bonds, width)
    return out["priority"] if out["flags"] == CANONICAL else W.priority(n, atoms, nb, bonds, width)


def graph_write(atoms, bonds, class_id, W_=128, width=MAX_WIDTH):
    """molwrite_ref.write_arrays of lists cut to their counts, walked in write_priority()"""
    import molwrite_ref as W
    n, nb = len(atoms), len(bonds)
    return W.write_arrays(n, atoms, nb, bonds, write_priority(n, atoms, nb, bonds, width), class_id, W_, width)


def respell(s):
    """mol_respell(canonical=True) of a string as characters ("" for no molecule)"""
    import molwrite_ref as W
    _, _, atoms, bonds = K.graph(s)
    out = string_canon(s)
    prio = out["priority"] if out["flags"] == CANONICAL else W.priority(len(atoms), atoms, len(bonds), bonds)
    return W.write_arrays(len(atoms), atoms, len(bonds), bonds, prio, W.ASCII_CLASS_ID, 128)["text"]
