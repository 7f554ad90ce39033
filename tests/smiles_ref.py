"""String-level reference of mdt_smiles_check (csrc/k_smiles.hip): plain Python written from the rule set in include/mdt_hip.h,
sharing no code and no table with the package.  check(s) -> (status, position).

Also the three tables of verdicts the rule set was agreed on, and the recipe of mutated rows the GPU test compares on."""
import random
import re

OK, MALFORMED, OVERVALENT = 0, 32, 64

ELEMENTS = set(re.findall(r"[A-Z][a-z]?", (
    "HHeLiBeBCNOFNeNaMgAlSiPSClArKCaScTiVCrMnFeCoNiCuZnGaGeAsSeBrKrRbSrYZrNbMoTcRuRhPdAgCdInSnSbTeIXeCsBaLaCePrNdPmSmEuGdTbDyHoEr"
    "TmYbLuHfTaWReOsIrPtAuHgTlPbBiPoAtRnFrRaAcThPaUNpPuAmCmBkCfEsFmMdNoLrRfDbSgBhHsMtDsRgCnNhFlMcLvTsOg")))
assert len(ELEMENTS) == 118
ORGANIC = set("BCNOPSFI")
AROMATIC = set("bcnops")
BOND_ORDER = {"-": 1, "=": 2, "#": 3, "$": 4, ":": 1, "/": 1, "\\": 1}
MAX_VALENCE = {"B": 3, "C": 4, "N": 3, "O": 2, "P": 5, "S": 6, "F": 1, "Cl": 1, "Br": 1, "I": 1}
DIGITS = set("0123456789")
UPPER = set("ABCDEFGHIJKLMNOPQRSTUVWXYZ")
LOWER = set("abcdefghijklmnopqrstuvwxyz")


class Violation(Exception):
    def __init__(self, position):
        self.position = position


def bracket_atom(s, j):
    """s[j] == '['.  -> index after the closing ']'; raises Violation."""
    n = len(s)

    def at(k):
        if k >= n:
            raise Violation(n)                                  # the row ends inside the bracket
        return s[k]
    k = j + 1
    while at(k) in DIGITS:                                      # isotope
        k += 1
    ch = at(k)
    if ch in UPPER:
        if k + 1 < n and s[k + 1] in LOWER and ch + s[k + 1] in ELEMENTS:
            k += 2
        elif ch in ELEMENTS:
            k += 1
        else:
            raise Violation(k)
    elif ch in AROMATIC or ch == "*":
        k += 1
    else:
        raise Violation(k)
    if at(k) == "@":                                            # chiral
        k += 1
        if at(k) == "@":
            k += 1
    if at(k) == "H":                                            # hcount
        k += 1
        if at(k) in DIGITS:
            k += 1
    if at(k) in "+-":                                           # charge
        sign = s[k]
        k += 1
        if at(k) == sign or at(k) in DIGITS:
            k += 1
    if at(k) == ":":                                            # class
        k += 1
        if at(k) not in DIGITS:
            raise Violation(k)
        while at(k) in DIGITS:
            k += 1
    if at(k) != "]":
        raise Violation(k)
    return k + 1


def check(s, max_valence=None):
    limits = dict(MAX_VALENCE, **(max_valence or {}))
    n = len(s)
    if n == 0:
        return OK, -1
    prev, before_bond = "START", None
    current, parents, pending = None, [], None
    rings = {}                                                  # number -> (opening atom, bond symbol or None)
    total, symbol = {}, {}                                      # per atom position: bond-order sum; judged symbol or None

    def join(a, b, order):
        total[a] += order
        total[b] += order
    try:
        j = 0
        while j < n:
            ch = s[j]
            atom = None                                         # (symbol or None, index after the atom)
            if ch == "[":
                atom = (None, bracket_atom(s, j))
            elif s[j:j + 2] in ("Cl", "Br"):
                atom = (s[j:j + 2], j + 2)
            elif ch in ORGANIC:
                atom = (ch, j + 1)
            elif ch in AROMATIC or ch == "*":
                atom = (None, j + 1)
            if atom is not None:
                total[j], symbol[j] = 0, atom[0]
                if prev not in ("START", "DOT"):
                    join(current, j, BOND_ORDER[pending] if pending else 1)
                current, pending, prev, j = j, None, "ATOM", atom[1]
            elif ch in BOND_ORDER:
                if prev not in ("ATOM", "CLOSE", "OPEN"):
                    raise Violation(j)
                before_bond, pending, prev, j = prev, ch, "BOND", j + 1
            elif ch in DIGITS or ch == "%":
                if not (prev in ("ATOM", "CLOSE") or (prev == "BOND" and before_bond in ("ATOM", "CLOSE"))):
                    raise Violation(j)
                if ch == "%":
                    for k in (j + 1, j + 2):
                        if k >= n:
                            raise Violation(n)
                        if s[k] not in DIGITS:
                            raise Violation(k)
                    number, last = int(s[j + 1:j + 3]), j + 2
                else:
                    number, last = int(ch), j
                if number not in rings:
                    rings[number] = (current, pending)
                else:
                    opener, sym = rings.pop(number)
                    if opener == current:
                        raise Violation(last)
                    if sym and pending and sym != pending and not {sym, pending} == {"/", "\\"}:
                        raise Violation(last)
                    join(opener, current, BOND_ORDER[sym or pending] if (sym or pending) else 1)
                pending, prev, j = None, "ATOM", last + 1
            elif ch == "(":
                if prev not in ("ATOM", "CLOSE"):
                    raise Violation(j)
                parents.append(current)
                prev, j = "OPEN", j + 1
            elif ch == ")":
                if prev not in ("ATOM", "CLOSE") or not parents:
                    raise Violation(j)
                current = parents.pop()
                prev, j = "CLOSE", j + 1
            elif ch == ".":
                if prev not in ("ATOM", "CLOSE") or parents:
                    raise Violation(j)
                prev, j = "DOT", j + 1
            else:
                raise Violation(j)
        if prev not in ("ATOM", "CLOSE") or parents or rings:
            raise Violation(n)
    except Violation as v:
        return MALFORMED, v.position
    over = [a for a in sorted(total) if symbol[a] is not None and total[a] > limits[symbol[a]]]
    return (OVERVALENT, over[0]) if over else (OK, -1)


# ----------------------------------------------------------------------------------------------------------------------
# the tables
# ----------------------------------------------------------------------------------------------------------------------
OK_TABLE = (r"C CC C=C C#N CCO CC(=O)O C1CC1 C1CC1C c1ccccc1 OC1CC1 C1=CC=CC=C1 CC(C)(C)C N#CC#N FC(F)(F)F ClCCl BrCBr C(Cl)Cl [NH4+] "
            r"[O-]C=O C[N+](C)(C)C [nH]1cccc1 c1cc[nH]c1 C12CC1C2 C1CC2CC12 C%10CC%10 C%10CC%10C1CC1 C/C=C/C C/C=C\C F/C=C/F "
            r"[C@H](N)(O)C [C@@H](N)(O)C C.C [Na+].[Cl-] C1.C1 CC(C)1CC1 C=1CC1 C1CC=1 C=1CC=1 O=C1CC1 N1C=CC=C1 CS(=O)(=O)C "
            r"CP(=O)(O)O C(=O)=O [13CH4] [2H]O[2H] [C:12]C C(C) C(C)(C) C(-C)C C(=O)C *C [*]C C$C CC1=CC(=O)C2CC2C1 OC1C2CC3CC1C3O2 "
            r"N#CC1(CC1)C#N CC1OC2CC1C2O O=CC1=CNC=N1 C1C2C3C1C1C2C31 CC12CC1C1OC21 c1cc2cc[nH]c2o1").split()
MALFORMED_TABLE = [
    ("(C)C", 0), ("C()", 2), ("C(", 2), ("C)", 1), ("C(C", 3), ("C((C))", 2), ("C1CC", 4), ("C11", 2), ("1CC1", 0), ("C=", 2),
    ("C==C", 2), ("=CC", 0), ("C=(C)C", 2), ("C(=)C", 3), ("C.", 2), (".C", 0), ("C..C", 2), ("C(.C)C", 2), ("C(C.C)C", 3),
    ("Cl1", 3), ("lC", 0), ("Cr", 1), ("CH4", 1), ("H", 0), ("C@C", 1), ("[C", 2), ("[]", 1), ("[Xx]", 1), ("[C@@@H]", 4),
    ("[CH23]", 4), ("[C+-]", 3), ("[C:]", 3), ("[C:a]", 3), ("C]", 1), ("C%1", 3), ("C%1C", 3), ("C%(10)", 2), ("C=1CC#1", 6),
    ("C-1CC=1", 6), ("Cx", 1), ("C C", 1), ("C(1CC1)", 2), ("C(=1CC1)", 3), ("C.1", 2), ("[12]", 3), ("[12", 3), ("[", 1),
    ("[H", 2), ("[C@", 3)]
OVERVALENT_TABLE = [
    ("C(C)(C)(C)(C)C", 0), ("CF(C)", 1), ("O(C)(C)C", 0), ("C=O=C", 2), ("N(C)(C)(C)C", 0), ("C#C#C", 2), ("ClC(Cl)Cl(C)", 7),
    ("C1(C)(C)(C)CC1C", 0), ("F1CC1", 0), ("C=C(=C)=C", 2), ("BrBrBr", 2), ("CCl(C)", 1), ("C=1(C)(C)CC=1", 0), ("N#N=O", 2)]
TABLES = ([(s, OK, -1) for s in OK_TABLE] + [(s, MALFORMED, p) for s, p in MALFORMED_TABLE] +
          [(s, OVERVALENT, p) for s, p in OVERVALENT_TABLE])

# every character of the tables, of the mutation alphabet and every digit: id = 1 + its place here ('x' and ' ' have ids so that
# they can occur)
ALPHABET = "CNOFcno()=#12[]H+-.l%/"
CHARS = sorted(set("".join(s for s, _, _ in TABLES) + ALPHABET + "0123456789"))


def mutated_rows(rows=4096, seed=11, width=32):
    """The mutated rows of the GPU test: base strings are the OK table's of at most 28 characters; row r gets r mod 3 mutations,
    each one of four equally likely kinds -- substitute, insert or delete one token from ALPHABET, or insert one of (F), (=O),
    (C)(C) after a random C/N/O/F -- and is truncated to ``width`` tokens."""
    rng = random.Random(seed)
    bases = [s for s in OK_TABLE if len(s) <= 28]
    out = []
    for r in range(rows):
        s = list(rng.choice(bases))
        for _ in range(r % 3):
            kind = rng.randrange(4)
            if kind == 0 and s:
                s[rng.randrange(len(s))] = rng.choice(ALPHABET)
            elif kind == 1:
                s.insert(rng.randrange(len(s) + 1), rng.choice(ALPHABET))
            elif kind == 2 and s:
                del s[rng.randrange(len(s))]
            elif kind == 3:
                spots = [i for i, ch in enumerate(s) if ch in "CNOF"]
                if spots:
                    i = rng.choice(spots) + 1
                    s[i:i] = list(rng.choice(["(F)", "(=O)", "(C)(C)"]))
        out.append("".join(s)[:width])
    return out
