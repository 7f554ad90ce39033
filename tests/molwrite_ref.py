"""Reference of mdt_mol_rank / mdt_mol_write (csrc/k_molwrite.hip): the definition in include/mdt_hip.h in plain Python ints and
lists on molkey_ref.graph() arrays (or on molnorm_ref's and molscaf_ref's), sharing no code and no table with the package.
priority() is the visiting priority of every atom -- the label it has under the root of its component whose rooted hash is the
smallest; write_arrays() spells graph arrays as a token row: a depth-first walk that takes start atoms and neighbours in ascending
(priority, index), ring numbers from the lowest free one, bond symbols where mdt_mol_graph's default would read another order."""
import numpy as np

import molkey_ref as K

MAX_WIDTH, MAX_TOKENS = 64, 128
WRITTEN, NO_FIT, NO_VOCABULARY, NOT_WRITABLE = 1, 2, 4, 8                    # the flags; exactly one is set for a molecule
SYMBOLS = "-=#$:/\\().[]%@+*"                                                # classes 63 .. 78
ORGANIC = {"B", "C", "N", "O", "P", "S", "F", "I", "Cl", "Br", "*", "b", "c", "n", "o", "p", "s"}
ORDER_SYMBOL = {1: "-", 2: "=", 3: "#", 4: "$", 5: ":"}


def char_class(ch):
    """The class byte of mdt_smiles_check for one character."""
    if "A" <= ch <= "Z":
        return 1 + ord(ch) - 65
    if "a" <= ch <= "z":
        return 27 + ord(ch) - 97
    if "0" <= ch <= "9":
        return 53 + int(ch)
    return 63 + SYMBOLS.index(ch) if ch in SYMBOLS else 0


def class_table(chars):
    """chars: {id: character}.  -> class_id [128]: the lowest id that stands for the class, 0 where none does."""
    table = [0] * 128
    for i in sorted(chars, reverse=True):
        table[char_class(chars[i])] = i
    table[0] = 0
    return table


def is_graph(n, nb, bonds, width):
    return 1 <= n <= width and 0 <= nb <= width and all(a < n and b < n for a, b, _ in bonds[:nb])


def components(n, bonds):
    """-> comp [n]: the lowest atom of the component of each atom in the ring graph (pairs a != b named by an entry)"""
    comp = list(range(n))
    changed = True
    while changed:
        changed = False
        for a, b, _ in bonds:
            low = min(comp[a], comp[b])
            if comp[a] != low or comp[b] != low:
                comp[a] = comp[b] = low
                changed = True
    return comp


def priority(n, atoms, nb, bonds, width=MAX_WIDTH):
    """mdt_mol_rank of one row -> [width] ints"""
    out = [0] * width
    if not is_graph(n, nb, bonds, width):
        return out
    atoms, bonds = list(atoms[:n]), list(bonds[:nb])
    seed = K.mix(np.array(atoms, dtype=np.uint64))
    lab = np.tile(seed[:, None], (1, n))                                     # [atom, root]
    lab[np.arange(n), np.arange(n)] = K.mix(seed ^ np.uint64(K.ROOT))
    with np.errstate(over="ignore"):
        if bonds:
            ends = np.array([(a, b) for a, b, _ in bonds], dtype=np.int64)
            ok = np.array([o * K.K & K.MASK for _, _, o in bonds], dtype=np.uint64)[:, None]
        for _ in range(n):
            acc = np.zeros((n, n), dtype=np.uint64)
            if bonds:
                np.add.at(acc, ends[:, 0], K.mix(lab[ends[:, 1]] + ok))
                np.add.at(acc, ends[:, 1], K.mix(lab[ends[:, 0]] + ok))
            lab = K.mix(lab ^ K.mix(acc))
        h = [int(x) for x in K.mix(lab).sum(axis=0, dtype=np.uint64)]
    comp = components(n, bonds)
    for a in range(n):
        root = min((r for r in range(n) if comp[r] == comp[a]), key=lambda r: (h[r], r))
        out[a] = int(lab[a, root])
    return out


def atom_text(d):
    """The characters of one atom word."""
    first, second = d & 31, d >> 5 & 31
    aromatic, bracket = d >> 10 & 1, d >> 11 & 1
    charge, h, isotope = d >> 12 & 31, d >> 17 & 15, d >> 21
    symbol = "*" if first == 26 else chr((97 if aromatic else 65) + first)
    if second:
        symbol += chr(96 + second)
    if not bracket and charge in (0, 9) and h == 0 and isotope == 0 and symbol in ORGANIC:
        return symbol
    text = "[" + (str(isotope) if isotope else "") + symbol
    if h:
        text += "H" + (str(h) if h >= 2 else "")
    if charge not in (0, 9):
        sign, size = ("+", charge - 9) if charge > 9 else ("-", 9 - charge)
        text += sign + (str(size) if size >= 2 else "")
    return text + "]"


def writable(n, atoms, bonds):
    pairs = set()
    for a, b, o in bonds:
        if a == b or frozenset((a, b)) in pairs or not 1 <= o <= 5:
            return False
        pairs.add(frozenset((a, b)))
    return all((d >> 17 & 15) <= 9 and (d >> 12 & 31) <= 18 and (d & 31) <= 26 and (d >> 5 & 31) <= 26 for d in atoms)


def number_text(k):
    return str(k) if k < 10 else "%%%02d" % k


def write_arrays(n, atoms, nb, bonds, prio, class_id, W, width=MAX_WIDTH):
    """mdt_mol_write of one row: n atoms (words) and nb bonds (a, b, order); prio: [>= n] ints or None.  -> dict(tokens [W], length,
    token_atom [W], flags, text: the characters of the T tokens whatever the flags say, owners [T], order: the atoms in the order
    they were visited)"""
    assert 1 <= W <= MAX_TOKENS
    out = dict(tokens=[0] * W, length=0, token_atom=[0] * W, flags=0, text="", owners=[], order=[])
    if not is_graph(n, nb, bonds, width):
        return out
    atoms, bonds = list(atoms[:n]), list(bonds[:nb])
    if not writable(n, atoms, bonds):
        out["flags"] = NOT_WRITABLE
        return out
    key = (lambda a: (prio[a], a)) if prio is not None else (lambda a: (0, a))
    aromatic = [d >> 10 & 1 for d in atoms]
    nbrs = [[] for _ in range(n)]
    order_of = {}
    for a, b, o in bonds:
        nbrs[a].append(b)
        nbrs[b].append(a)
        order_of[a, b] = order_of[b, a] = o
    for a in range(n):
        nbrs[a].sort(key=key)

    def symbol(a, b):
        o = order_of[a, b]
        both = aromatic[a] and aromatic[b]
        return "" if (o == 1 and not both) or (o == 5 and both) else ORDER_SYMBOL[o]
    # pass 1: the spanning forest
    seq, children, opens, closes, roots = {}, [[] for _ in range(n)], [[] for _ in range(n)], [[] for _ in range(n)], []

    def walk(a, parent):
        seq[a] = len(seq)
        for b in nbrs[a]:
            if b == parent:
                continue
            if b not in seq:
                children[a].append(b)
                walk(b, a)
            elif seq[b] < seq[a]:
                opens[b].append(a)
                closes[a].append(b)
    while len(seq) < n:
        roots.append(min((a for a in range(n) if a not in seq), key=key))
        walk(roots[-1], None)
    # pass 2: the emission
    text, owners, number, free = [], [], {}, set(range(1, 100))

    def put(chars, owner):
        text.extend(chars)
        owners.extend([owner] * len(chars))

    def emit(a):
        put(atom_text(atoms[a]), 1 + a)
        closed = []
        for b in sorted(closes[a], key=lambda b: seq[b]):
            put(number_text(number[b, a]), 1 + a)
            closed.append(number[b, a])
        for c in sorted(opens[a], key=lambda c: seq[c]):
            number[a, c] = min(free)
            free.discard(number[a, c])
            put(symbol(a, c) + number_text(number[a, c]), 1 + a)
        free.update(closed)
        for i, c in enumerate(children[a]):
            if i < len(children[a]) - 1:
                put("(", 1 + c)
            put(symbol(a, c), 1 + c)
            emit(c)
            if i < len(children[a]) - 1:
                put(")", 1 + c)
    for i, r in enumerate(roots):
        if i:
            put(".", 0)
        emit(r)
    T = len(text)
    out.update(length=T, text="".join(text), owners=owners, order=sorted(range(n), key=lambda a: seq[a]))
    ids = [class_id[char_class(ch)] for ch in text]
    if 0 in ids:
        out["flags"] = NO_VOCABULARY
    elif T > W:
        out["flags"] = NO_FIT
    else:
        out["flags"] = WRITTEN
        out["tokens"][:T] = ids
        out["token_atom"][:T] = owners
    return out


def at_width(out, W):
    """The answer at width W from the answer at a width where the row was written or did not fit (the tokens do not depend on the
    width; only whether they fit does)."""
    T = out["length"]
    if out["flags"] not in (WRITTEN, NO_FIT):
        return dict(out, tokens=[0] * W, token_atom=[0] * W)
    if T > W:
        return dict(out, tokens=[0] * W, token_atom=[0] * W, flags=NO_FIT)
    assert out["flags"] == WRITTEN
    return dict(out, tokens=out["tokens"][:T] + [0] * (W - T), token_atom=out["token_atom"][:T] + [0] * (W - T))


def graph_write(atoms, bonds, class_id, W=MAX_WIDTH, invariant=True, width=MAX_WIDTH):
    """write_arrays of lists cut to their counts, with the priority of the same arrays or without one"""
    n, nb = len(atoms), len(bonds)
    prio = priority(n, atoms, nb, bonds, width) if invariant else None
    return write_arrays(n, atoms, nb, bonds, prio, class_id, W, width)


_ROWS = {}


def string_write(s, class_id, W=MAX_WIDTH, invariant=True, width=MAX_WIDTH):
    """The answer for the graph of a string as mdt_mol_graph reads it (nothing for a row of status != 0)."""
    at = (s, tuple(class_id), W, invariant, width)
    if at not in _ROWS:
        _, _, atoms, bonds = K.graph(s)
        _ROWS[at] = graph_write(atoms, bonds, class_id, W, invariant, width)
    return _ROWS[at]


def ladder():
    """A 22-atom path with closure entries (i, 21 - i), i = 0..9: ten numbers open at once."""
    c = K.descriptor("C")
    return 64, 22, 31, [c] * 22, [(i, i + 1, 1) for i in range(21)] + [(i, 21 - i, 1) for i in range(10)]


def special_rows():
    """Graph arrays that no scan writes: molscaf_ref's, the %10 ladder, and each reason not to write."""
    c = K.descriptor("C")
    import molscaf_ref as C
    return C.special_rows() + [
        ladder(),
        (8, 3, 2, [c] * 3, [(0, 1, 6), (1, 2, 1)]), (8, 3, 2, [c] * 3, [(0, 1, 0), (1, 2, 1)]),       # an order outside 1..5
        (8, 2, 1, [c | 10 << 17 | 1 << 11, c], [(0, 1, 1)]), (8, 2, 1, [c, c | 19 << 12], [(0, 1, 1)]),   # H 10; a charge field of 19
        (8, 2, 1, [27, c], [(0, 1, 1)]), (8, 2, 1, [c | 27 << 5, c], [(0, 1, 1)]),                      # the letter fields
        (8, 3, 2, [c | 1 << 11, 26 | 1 << 10, c | 2047 << 21 | 9 << 17 | 1 << 11], [(0, 1, 5), (1, 2, 4)]),   # a charge field of 0; the longest text
        (64, 64, 64, [K.descriptor("Cl", True, -8, 9, 2047)] * 64, [(i, (i + 1) % 64, 2) for i in range(64)]),   # 64 atoms of 12 tokens
    ]


ASCII = {i: chr(i) for i in range(33, 127)}                                  # a vocabulary that has every character: id = code
ASCII_CLASS_ID = class_table(ASCII)


def respell(s, invariant=True):
    """The spelling of a string's graph as characters ("" for no molecule)."""
    return string_write(s, ASCII_CLASS_ID, MAX_TOKENS, invariant)["text"]
