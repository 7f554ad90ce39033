"""Reference of mdt_mol_scaffold (csrc/k_molscaf.hip): the definition in include/mdt_hip.h in plain Python sets and ints on
molkey_ref.graph() arrays (or on molnorm_ref.string_normal()'s), sharing no code and no table with the package.  Per row the
scaffold -- the 2-core of the ring graph, with mode bit 0 plus the atoms double-bonded to it -- as renumbered graph arrays, the map
from the row's atoms to the scaffold's and the flags.  TABLE holds molecules whose scaffold is written by hand as a spelling."""
import molh_ref as H
import molkey_ref as K
import molnorm_ref as N
import molring_ref as R

MAX_WIDTH = 64
EXOCYCLIC, GENERIC = 1, 2                                                    # the mode bits
MOLECULE, SCAFFOLD, WHOLE = 1, 2, 4                                          # the flag bits
PLAIN_C = K.descriptor("C")                                                  # what GENERIC writes for every kept atom
MODES = (0, 1, 2, 3)


def two_core(n, adj):
    """-> (the atoms left when, in rounds, every atom with at most one neighbour still present is removed at once, the rounds that
    removed an atom)"""
    alive, rounds = set(range(n)), 0
    while True:
        gone = {x for x in alive if len(adj[x] & alive) <= 1}
        if not gone:
            return alive, rounds
        alive -= gone
        rounds += 1


def weight(o):
    return o if 1 <= o <= 4 else 1


def scaffold_arrays(n, atoms, nb, bonds, mode, width=MAX_WIDTH):
    """-> dict(n, nb: the kept counts, atoms [width] ints, bonds [width] packed words, atom_map [width], flags, core, exo: sets of
    the row's atoms, rounds) for a row of n atoms and nb bonds (a, b, order).  The counts are given apart from the lists so that
    arrays no scan writes can be asked about."""
    assert mode in MODES
    out = dict(n=0, nb=0, atoms=[0] * width, bonds=[0] * width, atom_map=[0] * width, flags=0, core=set(), exo=set(), rounds=0)
    if not H.is_graph(n, nb, bonds, width):
        return out
    atoms, bonds = list(atoms[:n]), list(bonds[:nb])
    core, out["rounds"] = two_core(n, R.ring_graph(n, bonds))
    exo = set()
    if mode & EXOCYCLIC:
        for a, b, o in bonds:
            if a != b and o == 2:
                for x, y in ((a, b), (b, a)):
                    if x not in core and y in core:
                        exo.add(x)
    kept = sorted(core | exo) if core else []
    new = {x: k for k, x in enumerate(kept)}
    gained = {x: 0 for x in kept}
    for a, b, o in bonds:
        if a != b:
            for x, y in ((a, b), (b, a)):
                if x in new and y not in new:
                    gained[x] += weight(o)
    for x in kept:
        d = atoms[x]
        if mode & GENERIC:
            d = PLAIN_C
        elif d >> 11 & 1:
            d = (d & ~(15 << 17)) | min(15, (d >> 17 & 15) + gained[x]) << 17
        out["atoms"][new[x]] = d
        out["atom_map"][x] = 1 + new[x]
    at = 0
    for a, b, o in bonds:
        if a != b and a in new and b in new:
            out["bonds"][at] = N.pack((new[a], new[b], 1 if mode & GENERIC else o))
            at += 1
    out.update(n=len(kept), nb=at, core=core, exo=exo if core else set())
    out["flags"] = MOLECULE | (SCAFFOLD if kept else 0) | (WHOLE if len(kept) == n else 0)
    return out


def unpacked(out):
    """(atoms, bonds as (a, b, order)) of an answer, cut to its counts: what molkey_ref.key() takes"""
    return out["atoms"][:out["n"]], [(w & 255, w >> 8 & 255, w >> 16) for w in out["bonds"][:out["nb"]]]


def input_arrays(s, normalize=False, width=MAX_WIDTH):
    """(n, atoms, nb, bonds as (a, b, order)) of a string as mdt_mol_graph writes them, or of its normal form"""
    if normalize:
        atoms, bonds = N.unpacked(N.string_normal(s, width))
    else:
        _, _, atoms, bonds = K.graph(s)
    return len(atoms), list(atoms), len(bonds), list(bonds)


_ROWS = {}


def string_scaffold(s, mode, normalize=False, width=MAX_WIDTH):
    """The answer for a string, with `natoms` / `nbonds`: the counts of the row itself."""
    at = (s, mode, normalize, width)
    if at not in _ROWS:
        n, atoms, nb, bonds = input_arrays(s, normalize, width)
        out = scaffold_arrays(n, atoms, nb, bonds, mode, width)
        out.update(natoms=n, nbonds=nb)
        _ROWS[at] = out
    return _ROWS[at]


def key_of(out):
    """molkey_ref's key of a scaffold (0: no scaffold)"""
    return K.key(*unpacked(out)) if out["n"] else 0


def scaffold_key(s, mode, normalize=False):
    return key_of(string_scaffold(s, mode, normalize))


def again(out, mode):
    """The scaffold of a scaffold."""
    atoms, bonds = unpacked(out)
    return scaffold_arrays(len(atoms), atoms, len(bonds), bonds, mode)


def special_rows():
    """Graph arrays that no scan writes: [(width, n, nb, atoms, bonds as (a, b, order))]."""
    c, ch = K.descriptor("C"), K.descriptor("C", True, 0, 1)
    ring = lambda m: [(i, (i + 1) % m, 1) for i in range(m)]  # noqa: E731
    return [
        (64, 64, 64, [c] * 64, ring(62) + [(0, 62, 2), (31, 63, 1)]),          # a 62-ring, one exocyclic atom, one substituent
        (64, 64, 64, [c] * 64, ring(64)),                                      # the whole row is one ring: every lane kept
        (8, 6, 8, [c] * 6, ring(4) + [(1, 2, 1), (0, 0, 2), (0, 4, 2), (5, 4, 2)]),   # listed twice; (x, x); =X with a tail
        (16, 8, 12, [K.descriptor("C", True, 0, 9)] * 3 + [c] * 5,              # the H field clamps at 15: 9 + 4 + 3; 9 + 2 + 2; 9 + 1
         ring(3) + [(0, 3, 4), (3, 0, 3), (1, 4, 2), (4, 1, 2), (2, 5, 1), (2, 6, 1), (2, 7, 1), (5, 5, 1), (6, 7, 65535)]),
        (8, 5, 6, [ch, c, ch, c, c], ring(3) + [(0, 3, 0), (2, 4, 7), (4, 2, 5)]),    # orders outside 1..4 weigh 1
        (8, 4, 5, [c] * 4, [(0, 1, 1), (1, 2, 1), (2, 0, 1), (3, 0, 2), (3, 1, 2)]),  # double-bonded to two core atoms: in the core
        (8, 65, 0, [], []), (8, 2, 65, [c] * 2, []), (8, -1, 0, [], []), (8, 2, -1, [c] * 2, []), (8, 0, 0, [], []),
        (8, 3, 2, [c] * 3, [(0, 3, 1), (1, 2, 1)]),                            # a bond naming a missing atom: no molecule
        (28, 8, 28, [c] * 8, [(i, j, 1) for i in range(8) for j in range(i)]),  # the complete graph on 8 atoms
        (1, 1, 1, [c], [(0, 0, 1)]), (2, 2, 2, [c] * 2, [(0, 1, 2), (1, 0, 2)]),   # one atom with (x, x); one edge listed twice
    ]


def select_classes(score, packed, length, N, G, K_, class_key, max_per_class, fps=None, sim_num=0, min_distance=1, reject=None):
    """mdt_screen_select_classes without a known set, on screen_ref.select()'s status bits: the eligible candidates of a group in
    (score, c) order; one is CLOSE (16) when a candidate kept before it is closer than min_distance edits, or at least sim_num /
    65536 similar (fps: fingerprints as ints, or None), or when its class_key is not 0 and max_per_class candidates kept before it
    carry the same one.  -> (status list (N * G), index G x K, count G)."""
    import molfp_ref as F
    import screen_ref as SR
    status = [int(s) | (int(reject[r]) if reject is not None else 0) for r, s in enumerate(SR.select(score, packed, length, N, G, K_)[0])]
    rows = [[int(t) for t in packed[r][:int(length[r])]] for r in range(N * G)]
    index, count = [], []
    for g in range(G):
        order = sorted((c for c in range(N) if status[c * G + g] == 0), key=lambda c: (float(score[c * G + g]), c))
        kept = []
        for c in order:
            r = c * G + g
            close = class_key[r] != 0 and sum(class_key[o * G + g] == class_key[r] for o in kept) >= max_per_class
            for o in kept:
                q = o * G + g
                close = close or (min_distance > 1 and F.edit_distance(rows[r], rows[q]) < min_distance)
                close = close or (fps is not None and F.at_least(*F.counts(fps[r], fps[q]), sim_num))
            if close:
                status[r] = 16
            elif len(kept) < K_:
                kept.append(c)
        index.append(kept + [-1] * (K_ - len(kept)))
        count.append(len(kept))
    return status, index, count


# molecule -> the spelling of its scaffold in mode 1 (EXOCYCLIC) and in mode 0, written by hand; None: no scaffold
TABLE = {
    "Cc1ccccc1": ("c1ccccc1", "c1ccccc1"),
    "CC(=O)c1ccccc1": ("c1ccccc1", "c1ccccc1"),
    "O=C(c1ccccc1)c1ccccc1": ("O=C(c1ccccc1)c1ccccc1", "C(c1ccccc1)c1ccccc1"),
    "O=C1CCCCC1": ("O=C1CCCCC1", "C1CCCCC1"),
    "CC(C)c1ccc(CC2CC2)cc1": ("c1ccc(CC2CC2)cc1", "c1ccc(CC2CC2)cc1"),
    "C1CC1.CCO": ("C1CC1", "C1CC1"),
    "C12CC12": ("C12CC12", "C12CC12"),
    "CC1CCC2(CC1)CCC(O)C2": ("C1CCC2(CC1)CCCC2", "C1CCC2(CC1)CCCC2"),          # a spiro system
    "Cc1ccc2cc(N)ccc2c1": ("c1ccc2ccccc2c1", "c1ccc2ccccc2c1"),                # a fused system
    "CCO": (None, None),
}
