"""Reference of mdt_mol_fp / mdt_fp_tanimoto_rows / mdt_fp_nearest / mdt_screen_select_similar (csrc/k_molfp.hip, csrc/k_screen.hip):
plain Python ints written from the definition in include/mdt_hip.h, sharing no code with the package.  molkey_ref supplies the
graph of a string, the splitmix64 step and the random graphs and spellings."""
import molkey_ref as K

MASK = (1 << 64) - 1
BITS, WORDS, SIM_DEN = 1024, 16, 65536
BOND_K = 0x100000001B3


def fingerprint(descriptors, bonds, radius=2, width=64):
    """-> the fingerprint as ONE Python int of 1024 bits (bit k of the int = bit k of the fingerprint).  bonds: (a, b, order).
    0 for no atoms, for counts a row of ``width`` cannot hold, and for a bond that names an atom the row does not have."""
    n = len(descriptors)
    if n < 1 or n > width or len(bonds) > width or any(a >= n or b >= n for a, b, _ in bonds):
        return 0
    deg = [0] * n
    for a, b, _ in bonds:
        deg[a] += 1
        deg[b] += 1
    ids = [K.mix(descriptors[a] | deg[a] << 32) for a in range(n)]
    bits = 0
    for r in range(radius + 1):
        for a in range(n):
            bits |= 1 << (ids[a] & (BITS - 1))
        if r == radius:
            break
        acc = [0] * n
        for a, b, order in bonds:
            acc[a] = (acc[a] + K.mix((ids[b] + order * BOND_K) & MASK)) & MASK
            acc[b] = (acc[b] + K.mix((ids[a] + order * BOND_K) & MASK)) & MASK
        ids = [K.mix(ids[a] ^ K.mix(acc[a])) for a in range(n)]
    return bits


_FPS = {}


def string_fp(s, radius=2):
    """The fingerprint of a string (0 unless it is an OK, non-empty row); each distinct (string, radius) is computed once."""
    if (s, radius) not in _FPS:
        _, _, atoms, bonds = K.graph(s)
        _FPS[s, radius] = fingerprint(atoms, bonds, radius)
    return _FPS[s, radius]


def words(bits):
    """The 16 uint64 words of a fingerprint: word w holds bits 64 w .. 64 w + 63."""
    return [(bits >> (64 * w)) & MASK for w in range(WORDS)]


def from_words(ws):
    return sum((int(w) & MASK) << (64 * i) for i, w in enumerate(ws))


def popcount(bits):
    return bin(bits).count("1")


def counts(a, b):
    """(inter, union) of two fingerprints."""
    inter = popcount(a & b)
    return inter, popcount(a) + popcount(b) - inter


def at_least(inter, union, sim_num):
    return union > 0 and inter * SIM_DEN >= sim_num * union


def nearest(q, known):
    """(index, inter, union): the lowest index of ``known`` that attains the largest inter / union (x / 0 = 0), exactly."""
    best = (0, 1, 0)                                                         # inter, union, index
    for k, b in enumerate(known):
        inter, union = counts(q, b)
        if union > 0 and inter * best[1] > best[0] * union:
            best = (inter, union, k)
    return (best[2],) + counts(q, known[best[2]])


def edit_distance(a, b):
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = cur
    return prev[-1]


def select_similar(score, rows, fps, N, G, K_, sim_num, min_distance=1, reject=None):
    """Greedy selection of mdt_screen_select_similar without a known set: rows[r] the compacted id list of row r = c * G + g,
    fps[r] its fingerprint (or None: no similarity test).  -> (status list (N * G), index G x K, count G)."""
    status = [0] * (N * G)
    index, count = [], []
    for g in range(G):
        for c in range(N):
            r = c * G + g
            st = 0
            if len(rows[r]) == 0:
                st |= 1
            if score[r] != score[r] or score[r] in (float("inf"), float("-inf")):
                st |= 2
            if any(rows[o * G + g] == rows[r] for o in range(c)):
                st |= 4
            if reject is not None:
                st |= reject[r]
            status[r] = st
        order = sorted((c for c in range(N) if status[c * G + g] == 0), key=lambda c: (score[c * G + g], c))
        kept = []
        for c in order:
            r = c * G + g
            close = False
            for o in kept:
                q = o * G + g
                if min_distance > 1 and edit_distance(rows[r], rows[q]) < min_distance:
                    close = True
                if fps is not None and at_least(*counts(fps[r], fps[q]), sim_num):
                    close = True
            if close:
                status[r] = 16
            elif len(kept) < K_:
                kept.append(c)
        index.append(kept + [-1] * (K_ - len(kept)))
        count.append(len(kept))
    return status, index, count
