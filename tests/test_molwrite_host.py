"""No GPU: the definition of the SMILES writer (include/mdt_hip.h, mdt_mol_rank / mdt_mol_write) on its reference
(tests/molwrite_ref.py) -- the hand spellings, the round trip through molkey_ref.graph(), one row per graph, symmetric molecules
under renumbering, the fixed point of the index order, every flag, the %10 ladder, token_atom and the scaffold mask -- and the
plumbing: C exports and argument checks, the class_id table, op schemas and shape inference, the refusals, and the launch order of
the four public calls on a recording library."""
import contextlib
import os
import random
import re

import pytest
import torch

import molkey_ref as K
import molnorm_ref as N
import molscaf_ref as C
import molwrite_ref as W
import smiles_ref as S
from conftest import ROOT
import moleculediffusiontransformer_amd as M
from moleculediffusiontransformer_amd import ops, runtime as rt

HAND = {"CCO": "OCC", "CC1CC1": "C1CC1C", "Cc1ccccc1": "c1ccc(cc1)C", "CC(=O)O": "OC(C)=O", "c1ccc(cc1)-c1ccccc1": "c1(ccccc1)-c1ccccc1",
        "C%12CCCCC%12": "C1CCCCC1", "[NH4+].[Cl-]": "[Cl-].[NH4+]", "c1cc[nH]c1": "[nH]1cccc1", "[13CH3]C": "C[13CH3]"}
# symmetric molecules: cubane, cuneane, prismane, adamantane, biphenyl, naphthalene, anthracene, pyrene, spiro[5.5]undecane,
# norbornane, bicyclo[2.2.2]octane, citric acid, two rings, two cubanes, ...
SYMMETRIC = ["C12C3C4C1C5C2C3C45", "C12C3C1C1C4C2C3C41", "C12C3C1C1C2C31", "C1C2CC3CC1CC(C2)C3", "c1ccc(cc1)-c1ccccc1", "c1ccc2ccccc2c1",
             "c1ccc2cc3ccccc3cc2c1", "c1cc2ccc3cccc4ccc(c1)c2c34", "C1CCC2(CC1)CCCCC2", "C1CC2CCC1C2", "C1CC2CCC1CC2",
             "OC(=O)CC(O)(CC(O)=O)C(O)=O", "C1CC1.C1CC1", "C12C3C4C1C5C2C3C45.C12C3C4C1C5C2C3C45",
             "c1ccccc1", "C1CCCCC1", "CC(C)(C)C", "C1CC1", "C12C3C1C23", "Cc1cc(C)cc(C)c1", "Cc1ccc(C)cc1", "ClC(Cl)(Cl)Cl",
             "FC(F)(F)C(F)(F)F", "O=C=O", "C1COCCO1", "C1CCC2CCCCC2C1", "C1CCCCC1C1CCCCC1", "CC.CC.CC", "c1ccc2c(c1)c1ccccc1c1ccccc21",
             "[NH4+].[Cl-].[NH4+].[Cl-]"]
CORONENE = "c1cc2ccc3ccc4ccc5ccc6ccc1c1c2c3c4c5c61"                            # where the index breaks a tie differently: a limit


@pytest.fixture(scope="module")
def spelled():
    return K.random_spellings()


def renumbered(atoms, bonds, rng):
    """The same graph under a random numbering of its atoms, a random order of its entries and random orientations."""
    to = list(range(len(atoms)))
    rng.shuffle(to)
    new_atoms = [0] * len(atoms)
    for a, d in enumerate(atoms):
        new_atoms[to[a]] = d
    new_bonds = [(to[a], to[b], o) if rng.random() < 0.5 else (to[b], to[a], o) for a, b, o in bonds]
    rng.shuffle(new_bonds)
    return new_atoms, new_bonds


def same_graph(out, atoms, bonds):
    """Does the written text read back (molkey_ref.graph) to the input's atoms in the order of `order`, and to its bonds?"""
    status, _, got_atoms, got_bonds = K.graph(out["text"])
    new = {a: k for k, a in enumerate(out["order"])}
    want = sorted((min(new[a], new[b]), max(new[a], new[b]), o) for a, b, o in bonds)
    return (status == 0 and got_atoms == [atoms[a] for a in out["order"]] and
            sorted((min(a, b), max(a, b), o) for a, b, o in got_bonds) == want)


# ---------------------------------------------------------------------------------------------------------------------
# the definition on the reference
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", sorted(HAND))
def test_the_hand_spellings(s):
    assert W.respell(s) == HAND[s]
    assert K.string_key(W.respell(s)) == K.string_key(s) != 0


def test_the_random_spellings_round_trip_and_come_out_as_one_row_per_graph(spelled):
    round_trip = one = one_as_numbered = longer = longest = 0
    for g, sp in spelled:
        rows = []
        for s in sp:
            _, _, atoms, bonds = K.graph(s)
            out = W.string_write(s, W.ASCII_CLASS_ID, 64)
            assert out["flags"] == W.WRITTEN and out["length"] == len(out["text"]) <= 64, s
            round_trip += same_graph(out, atoms, bonds) and K.string_key(out["text"]) == K.string_key(s)
            longer += len(out["text"]) > len(s)
            longest = max(longest, len(out["text"]))
            rows.append(out["text"])
        one += len(set(rows)) == 1
        one_as_numbered += len({W.respell(s, False) for s in sp}) == 1
    print("round trips %d, one row %d, as numbered %d, longer %d, longest %d" % (round_trip, one, one_as_numbered, longer, longest))
    assert (round_trip, one, one_as_numbered, longer, longest) == (2000, 500, 69, 108, 55)


@pytest.mark.parametrize("s", SYMMETRIC)
def test_a_symmetric_molecule_has_one_row_under_renumbering(s):
    status, _, atoms, bonds = K.graph(s)
    assert status == 0
    rng = random.Random(len(s))
    rows = {W.graph_write(*renumbered(atoms, bonds, rng), W.ASCII_CLASS_ID, 128)["text"] for _ in range(24)}
    assert len(rows) == 1 and K.string_key(min(rows)) == K.string_key(s), rows


def test_the_table_of_symmetric_molecules_and_a_limit():
    assert len(SYMMETRIC) == len(set(SYMMETRIC)) == 30
    # not a canonical form: ties of the priority are broken by the index, and in coronene two numberings break one differently
    _, _, atoms, bonds = K.graph(CORONENE)
    rng = random.Random(11)
    rows = {W.graph_write(*renumbered(atoms, bonds, rng), W.ASCII_CLASS_ID, 128)["text"] for _ in range(24)}
    assert len(rows) >= 1 and all(K.string_key(r) == K.string_key(CORONENE) for r in rows)
    print("coronene: %d rows under 24 renumberings" % len(rows))


def test_larger_random_graphs_come_out_as_one_row():
    spelled = K.random_spellings(graphs=200, spellings=4, seed=7, max_atoms=40)
    assert max(len(g.atoms) for g, _ in spelled) > 20
    for _, sp in spelled:
        assert len({W.respell(s) for s in sp}) == 1, sp


def test_the_index_order_is_a_fixed_point(spelled):
    rows = [s for _, sp in spelled for s in sp[:1]] + list(N.TABLE) + list(C.TABLE)
    for s in rows:
        once = W.respell(s, False)
        assert W.respell(once, False) == once, s
        _, _, atoms, bonds = K.graph(once)                                   # and reads back to the numbering it was written from
        assert W.graph_write(atoms, bonds, W.ASCII_CLASS_ID, 128, False)["order"] == list(range(len(atoms)))


def test_each_flag_from_a_hand_built_graph():
    c = K.descriptor("C")
    full = W.ASCII_CLASS_ID
    write = lambda atoms, bonds, table=full, width=64: W.write_arrays(len(atoms), atoms, len(bonds), bonds, None, table, width)  # noqa: E731
    for atoms, bonds in (([c] * 2, [(0, 1, 1), (1, 0, 1)]), ([c] * 2, [(0, 1, 1), (1, 1, 1)]), ([c] * 2, [(0, 1, 6)]), ([c] * 2, [(0, 1, 0)]),
                         ([c | 1 << 11 | 10 << 17, c], [(0, 1, 1)]), ([c | 19 << 12], []), ([27], []), ([c | 27 << 5], [])):
        out = write(atoms, bonds)
        assert out["flags"] == W.NOT_WRITABLE and out["length"] == 0 and not any(out["tokens"] + out["token_atom"]), (atoms, bonds)
    assert write([c] * 3, [(0, 3, 1)])["flags"] == 0 and write([], [])["flags"] == 0          # no molecule: not "not writable"
    without = lambda chars: W.class_table({i: ch for i, ch in W.ASCII.items() if ch not in chars})  # noqa: E731
    ring, ammonium = K.graph("C1CC1")[2:], K.graph("[NH4+]")[2:]
    assert write(*ring)["flags"] == W.WRITTEN and write(*ring, without("1"))["flags"] == W.NO_VOCABULARY
    out = write(*ammonium, without("["))
    assert out["flags"] == W.NO_VOCABULARY and out["length"] == 6 and not any(out["tokens"] + out["token_atom"])
    assert write(*ammonium, without("%"))["flags"] == W.WRITTEN
    for width, flags in ((4, W.NO_FIT), (5, W.WRITTEN), (1, W.NO_FIT)):
        out = write(*ring, full, width)
        assert out["flags"] == flags and out["length"] == 5 and len(out["tokens"]) == width
        assert (out["tokens"] == [ord(ch) for ch in "C1CC1"]) == (flags == W.WRITTEN)
    assert write(*ring, without("1"), 2)["flags"] == W.NO_VOCABULARY          # the precedence: 8, then 4, then 2, then 1
    assert write([c] * 2, [(0, 1, 6)], without("C"), 1)["flags"] == W.NOT_WRITABLE
    # the atom text: what needs brackets, and what a field of 0 or 9 writes
    text = lambda d: write([d], [])["text"]  # noqa: E731
    assert [text(K.descriptor(x)) for x in ("C", "Cl", "Br", "*", "n", "I")] == ["C", "Cl", "Br", "*", "n", "I"]
    assert text(K.descriptor("C", True)) == "[C]" and text(K.descriptor("Si")) == "[Si]" and text(K.descriptor("C", False, 0, 1)) == "[CH]"
    assert text(K.descriptor("N", True, 1, 4)) == "[NH4+]" and text(K.descriptor("O", True, -1)) == "[O-]" and text(K.descriptor("Fe", True, 2)) == "[Fe+2]"
    assert text(K.descriptor("C", True, -8, 9, 2047)) == "[2047CH9-8]" and text(K.descriptor("C", True, 9, 0, 13)) == "[13C+9]"
    assert text(c & ~(31 << 12)) == "C" and text((c | 1 << 11) & ~(31 << 12)) == "[C]"      # a charge field of 0 writes nothing
    assert text(K.descriptor("f")) == "[f]" and text(26 | 1 << 10) == "*"
    # the bond symbol: the exact inverse of the reader's default
    a, ar = K.descriptor("C"), K.descriptor("c")
    pairs = {(a, a, 1): "CC", (a, a, 2): "C=C", (a, a, 3): "C#C", (a, a, 4): "C$C", (a, a, 5): "C:C", (ar, ar, 5): "cc", (ar, ar, 1): "c-c",
             (ar, a, 1): "cC", (ar, a, 5): "c:C", (ar, ar, 2): "c=c"}
    for (x, y, o), want in pairs.items():
        assert write([x, y], [(0, 1, o)])["text"] == want


def test_the_ladder_writes_percent_ten():
    c = K.descriptor("C")
    bonds = [(i, i + 1, 1) for i in range(21)] + [(i, 21 - i, 1) for i in range(10)]
    out = W.write_arrays(22, [c] * 22, 31, bonds, None, W.ASCII_CLASS_ID, 64)
    assert out["flags"] == W.WRITTEN and out["text"] == "".join("C%s" % W.number_text(k) for k in range(1, 11)) + "CC" + \
        "".join("C%s" % W.number_text(k) for k in range(10, 0, -1))
    assert out["text"].count("%10") == 2 and out["text"].count("%") == 2 and out["length"] == 46
    assert K.key(*K.graph(out["text"])[2:]) == K.key([c] * 22, bonds)
    assert W.write_arrays(22, [c] * 22, 31, bonds, None, W.class_table({i: ch for i, ch in W.ASCII.items() if ch != "%"}), 64)["flags"] == W.NO_VOCABULARY
    ranked = W.graph_write([c] * 22, bonds, W.ASCII_CLASS_ID, 64)
    assert ranked["flags"] == W.WRITTEN and K.key(*K.graph(ranked["text"])[2:]) == K.key([c] * 22, bonds)


def test_token_atom(spelled):
    for s in [sp[0] for _, sp in spelled[:200]] + list(C.TABLE) + list(HAND):
        _, _, atoms, bonds = K.graph(s)
        out = W.string_write(s, W.ASCII_CLASS_ID, 64)
        if s == "C12CC12":                                                   # two closures between one pair of atoms: not writable
            assert out["flags"] == W.NOT_WRITABLE and not any(out["token_atom"])
            continue
        text, owners = out["text"], out["owners"]
        assert out["token_atom"][:out["length"]] == owners and not any(out["token_atom"][out["length"]:])
        first = []
        for o in owners:
            if o and o - 1 not in first:
                first.append(o - 1)
        assert first == out["order"] and sorted(first) == list(range(len(atoms)))
        for j, (ch, o) in enumerate(zip(text, owners)):
            assert (o == 0) == (ch == "."), (s, j)
            if ch in "(-=#$:" and text[j + 1] not in "0123456789%":           # what leads to an atom goes with that atom
                nxt = next(k for k in range(j + 1, len(text)) if text[k] not in "(-=#$:")
                assert owners[nxt] == o, (s, j)
            if ch in "0123456789%" or ch == "]":                              # ring tokens and the text go with the atom before
                assert owners[j - 1] == o, (s, j)
        depth = []
        for ch, o in zip(text, owners):                                      # '(' and its ')' have one owner
            if ch == "(":
                depth.append(o)
            elif ch == ")":
                assert depth.pop() == o, s


def reference_keep(s, normalize=False, exocyclic=True, width=64):
    """scaffold_keep() on the references: the respelled row, and the mask of the tokens of the scaffold's atoms"""
    n, atoms, nb, bonds = C.input_arrays(s, normalize)
    out = W.graph_write(atoms, bonds, W.ASCII_CLASS_ID, width)
    atom_map = C.scaffold_arrays(n, atoms, nb, bonds, 1 if exocyclic else 0)["atom_map"]
    return out, [o != 0 and atom_map[o - 1] != 0 for o in out["token_atom"]]


@pytest.mark.parametrize("s", sorted(C.TABLE))
def test_the_scaffold_mask_on_the_scaffold_table(s):
    for mode, scaffold in zip((1, 0), C.TABLE[s]):
        out, mask = reference_keep(s, exocyclic=bool(mode))
        if s == "C12CC12":                                                   # not writable: nothing is kept
            assert out["flags"] == W.NOT_WRITABLE and not any(mask)
            continue
        assert out["flags"] == W.WRITTEN
        kept = {o - 1 for o, m in zip(out["token_atom"], mask) if m}
        want = C.string_scaffold(s, mode)
        assert kept == {a for a in range(want["natoms"]) if want["atom_map"][a]} and (scaffold is None) == (not any(mask))
        if scaffold is None:
            continue
        text = "".join(ch for ch, m in zip(out["text"], mask) if m)           # the kept tokens hold every atom of the scaffold
        letters = lambda t: sorted(ch for ch in t if ch.isalpha())  # noqa: E731
        assert letters(text) == letters(scaffold), (s, text)
    out, mask = reference_keep("Cc1ccccc1")
    assert out["text"] == "c1ccc(cc1)C" and "".join("x" if m else "." for m in mask[:11]) == "xxxxxxxxxx." and not any(mask[11:])
    out, mask = reference_keep("CC(=O)c1ccccc1")                              # what leads to a pruned atom is not kept
    assert out["text"] == "c1c(cccc1)C(=O)C" and "".join("x" if m else "." for m in mask[:16]) == "xxxxxxxxxx......"
    out, mask = reference_keep("O=C1CCCCC1")                                 # the exocyclic =O: kept with its symbol, or neither
    assert out["text"] == "C1CCCCC1=O" and all(mask[:10]) and sum(reference_keep("O=C1CCCCC1", exocyclic=False)[1]) == 8


# ---------------------------------------------------------------------------------------------------------------------
# the plumbing
# ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_the_library_exports_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "mdt_hip.h")).read()
    lib = rt.load_library()
    for name, arity in (("mdt_mol_rank", 8), ("mdt_mol_write", 14)):
        assert re.search(r"\bint %s\s*\(" % name, hdr) and name in rt.SYMBOLS and hasattr(lib, name)
        assert len(rt.SYMBOLS[name][1]) == arity
    assert int(re.search(r"#define MDT_ABI_VERSION (\d+)", hdr).group(1)) == rt.ABI_VERSION == 5 == lib.mdt_abi_version()
    for name, value in (("WRITTEN", W.WRITTEN), ("NO_FIT", W.NO_FIT), ("NO_VOCABULARY", W.NO_VOCABULARY), ("NOT_WRITABLE", W.NOT_WRITABLE)):
        assert int(re.search(r"\bMDT_MOLW_%s = (\d+)" % name, hdr).group(1)) == value == getattr(rt, "MOLW_" + name)
    assert int(re.search(r"\bMDT_MOLW_MAX_WIDTH = (\d+)", hdr).group(1)) == W.MAX_TOKENS == rt.MOLW_MAX_WIDTH
    flat = " ".join(hdr.replace(" * ", " ").split())
    for phrase in ("OPENS at b and CLOSES at a", "the lowest free number in 1..99", "become free only after a's own numbers are written",
                   "the exact inverse of mdt_mol_graph's rule", "A closure's symbol stands at its opening end only",
                   "a field of 9 or 0 writes nothing", "RDKit's canonical SMILES", "a canonical form", "One root per component",
                   "'(' and its ')' belong to the first atom inside", "there is no step cap"):
        assert phrase in flat, phrase
    assert "k_molwrite.hip" in [s for s, _ in __import__("moleculediffusiontransformer_amd.build", fromlist=["SOURCES"]).SOURCES]
    src = open(os.path.join(ROOT, "moleculediffusiontransformer_amd", "csrc", "k_molwrite.hip")).read()
    for used in ("mol_root_hash(", "molw_atom_tokens(", "molw_atom_ok(", "mol_graph_ok_wave(", "mdt_molwrite.h", "mdt_finish(", "__ballot("):
        assert used in src, used
    shared = open(os.path.join(ROOT, "moleculediffusiontransformer_amd", "csrc", "mdt_molwrite.h")).read()
    scan = open(os.path.join(ROOT, "moleculediffusiontransformer_amd", "csrc", "mdt_smiles_scan.h")).read()
    assert "uint64_t mol_root_hash(" not in src + shared and scan.count("uint64_t mol_root_hash(") == 1   # shared, not copied
    assert "molw_row(" in shared and "molw_rank_row(" in shared and "mdt_molrow.h" in shared
    for helper in ("mol_popc", "mol_lowest", "mol_all", "mol_ring_adj", "mol_component"):                  # reused, not copied
        assert helper + "(" in shared and re.search(r"\b(int|void|uint64_t) " + helper + r"\(", shared) is None, helper
    for f in (M.mol_write, M.mol_respell, M.scaffold_tokens, M.scaffold_keep):
        assert "NOT RDKit's canonical SMILES" in " ".join(f.__doc__.split()), f.__name__
    readme = " ".join(open(os.path.join(ROOT, "README.md")).read().split())
    assert "mol_respell" in readme and "scaffold_keep" in readme and "NOT RDKit's canonical SMILES" in readme


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = rt.load_library()

    def rank(L=32, R_=5, p=8, out=8, **one):
        a = dict(natoms=p, atoms=p, nbonds=p, bonds=p, priority=out)
        a.update(one)
        return lib.mdt_mol_rank(a["natoms"], a["atoms"], a["nbonds"], a["bonds"], L, R_, a["priority"], 0)

    def write(L=32, R_=5, W_=64, p=8, out=8, priority=0, **one):
        a = dict(natoms=p, atoms=p, nbonds=p, bonds=p, class_id=p, tokens=out, length=out, token_atom=out, flags=out)
        a.update(one)
        return lib.mdt_mol_write(a["natoms"], a["atoms"], a["nbonds"], a["bonds"], priority, L, R_, a["class_id"], W_, a["tokens"], a["length"],
                                 a["token_atom"], a["flags"], 0)
    for call, name in ((rank, b"mdt_mol_rank"), (write, b"mdt_mol_write")):
        cases = [(dict(L=0), b"L <= 64"), (dict(L=65), b"L <= 64"), (dict(R_=-1), b"R >= 0"), (dict(p=0), b"null"), (dict(out=0), b"null")]
        if call is write:
            cases += [(dict(W_=0), b"W <= 128"), (dict(W_=129), b"W <= 128")]
            cases += [({k: 0}, b"null") for k in ("natoms", "atoms", "nbonds", "bonds", "class_id", "tokens", "length", "token_atom", "flags")]
        for kw, what in cases:
            assert call(**kw) == 2, kw
            assert what in lib.mdt_last_error() and name in lib.mdt_last_error(), (kw, lib.mdt_last_error())
        assert call(R_=0) == 0 and call(R_=0, p=0, out=0) == 0               # nothing to do: nothing is launched or read
        assert call(R_=0, L=65) != 0 and call(R_=0, L=0) != 0
    assert write(R_=0, W_=129) != 0 and write(R_=0, W_=0) != 0


def vocabulary():
    return M.SmilesVocabulary([None] + S.CHARS)


def test_the_class_id_table():
    v = M.SmilesVocabulary([None, "C", "c", "C", "1", "%", None, "(", "1", "é"])
    assert v.class_id.dtype.name == "uint8" and v.class_id.shape == (128,)
    want = [0] * 128
    want[3], want[29], want[54], want[75], want[70] = 1, 2, 4, 5, 7           # of two ids for one character the lower one encodes
    assert v.class_id.tolist() == want and v.encode(["C1"], 2).tolist() == [[1, 4]]
    assert v.class_id_on("cpu") is v.class_id_on("cpu") and v.class_id_on("cpu").tolist() == want
    full = M.SmilesVocabulary(dict(W.ASCII))
    assert full.class_id.tolist() == W.ASCII_CLASS_ID
    assert len(vocabulary().on("cpu")) == 3                                   # the three tables of the readers stay three


def test_op_schemas_and_shape_inference():
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert str(torch.ops.mdt.mol_rank.default._schema) == "mdt::mol_rank(Tensor natoms, Tensor atoms, Tensor nbonds, Tensor bonds) -> Tensor"
    assert str(torch.ops.mdt.mol_write.default._schema) == \
        ("mdt::mol_write(Tensor natoms, Tensor atoms, Tensor nbonds, Tensor bonds, Tensor? priority, Tensor class_id, SymInt width) -> "
         "(Tensor, Tensor, Tensor, Tensor)")
    with FakeTensorMode():
        n, rows = torch.empty(15, dtype=torch.int32), torch.empty(15, 40, dtype=torch.int32)
        p = torch.ops.mdt.mol_rank(n, rows, n, rows)
        assert (tuple(p.shape), p.dtype) == ((15, 40), torch.int64)
        out = torch.ops.mdt.mol_write(n, rows, n, rows, p, torch.empty(128, dtype=torch.uint8), 100)
        assert [(tuple(t.shape), t.dtype) for t in out] == [((15, 100), torch.int32), ((15,), torch.int32), ((15, 100), torch.uint8),
                                                            ((15,), torch.uint8)]
    n, rows = torch.zeros(3, dtype=torch.int32), torch.zeros(3, 4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU implementation"):          # no CPU implementation behind the ops
        torch.ops.mdt.mol_rank(n, rows, n, rows)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        torch.ops.mdt.mol_write(n, rows, n, rows, None, torch.zeros(128, dtype=torch.uint8), 4)


class Recorder:
    """Stands for libmdt_hip.so: every launch is appended to ``log``."""

    def __init__(self):
        self.log = []

    def __getattr__(self, name):
        if not name.startswith("mdt_"):
            raise AttributeError(name)
        return lambda *a: self.log.append((name,) + a) or 0


@pytest.fixture
def rec(monkeypatch):
    rec = Recorder()
    monkeypatch.setattr(rt, "load_library", lambda *a, **k: rec)
    monkeypatch.setattr(rt, "current_stream", lambda: 0)
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    monkeypatch.setattr(ops, "_hip", lambda *t: torch.device("cpu"))         # (the device guard: there is no device here)
    return rec


R_, L_ = 7, 16
FORM = ["mdt_mol_hydrogens", "mdt_mol_rings", "mdt_mol_normalize"]


def names(rec):
    return [e[0] for e in rec.log]


def test_the_ops_on_a_recording_library(rec):
    n, rows = torch.zeros(R_, dtype=torch.int32), torch.zeros(R_, L_, dtype=torch.int32)
    table = torch.zeros(128, dtype=torch.uint8)
    p = torch.ops.mdt.mol_rank(n, rows, n, rows)
    out = torch.ops.mdt.mol_write(n, rows, n, rows, p, table, 100)
    torch.ops.mdt.mol_write(n, rows, n, rows, None, table, 1)
    assert names(rec) == ["mdt_mol_rank", "mdt_mol_write", "mdt_mol_write"]
    assert rec.log[0][5:7] == (L_, R_) and rec.log[0][7] == p.data_ptr()
    assert rec.log[1][5] == p.data_ptr() and rec.log[1][6:8] == (L_, R_) and rec.log[1][9] == 100 and rec.log[1][10] == out[0].data_ptr()
    assert rec.log[2][5] == 0 and rec.log[2][9] == 1                        # no priority: NULL
    rec.log.clear()
    none, wide = torch.zeros(0, dtype=torch.int32), torch.zeros(0, L_, dtype=torch.int32)
    assert tuple(torch.ops.mdt.mol_rank(none, wide, none, wide).shape) == (0, L_)        # R == 0 launches nothing
    out = torch.ops.mdt.mol_write(none, wide, none, wide, None, table, 9)
    assert [tuple(t.shape) for t in out] == [(0, 9), (0,), (0, 9), (0,)] and rec.log == []
    too_wide = torch.zeros(R_, 65, dtype=torch.int32)
    for call in (lambda: torch.ops.mdt.mol_rank(n, too_wide, n, too_wide), lambda: torch.ops.mdt.mol_write(n, too_wide, n, too_wide, None, table, 64),
                 lambda: torch.ops.mdt.mol_write(n, rows, n, rows, None, table, 129), lambda: torch.ops.mdt.mol_write(n, rows, n, rows, None, table, 0),
                 lambda: torch.ops.mdt.mol_write(n, rows, n, rows, p[:, :5], table, 64), lambda: torch.ops.mdt.mol_write(n, rows, n, rows, p.int(), table, 64),
                 lambda: torch.ops.mdt.mol_write(n, rows, n, rows, None, table[:64], 64), lambda: torch.ops.mdt.mol_rank(n, rows.long(), n, rows)):
        with pytest.raises(RuntimeError, match="mdt::mol_"):
            call()
    assert rec.log == []                                                     # refused before any launch


def test_launch_order_of_the_public_calls(rec):
    tok, v = torch.ones(R_, L_, dtype=torch.long), vocabulary()
    head = ["mdt_tokens_compact", "mdt_mol_graph"]
    out = M.mol_respell(tok.to(torch.int16), v, "cpu")
    assert names(rec) == head + ["mdt_mol_rank", "mdt_mol_write"]
    graph, rank, write = rec.log[1:4]
    assert rank[1:5] == graph[8:12] == write[1:5] and write[5] == rank[7] and write[9] == L_ and write[8] == v.class_id_on("cpu").data_ptr()
    assert [tuple(t.shape) for t in out] == [(R_, L_), (R_,), (R_,), (R_,)] and all(t.dtype == torch.int64 for t in out)
    rec.log.clear()
    out = M.mol_respell(tok, v, "cpu", normalize=True, invariant=False, width=128)
    assert names(rec) == head + FORM + ["mdt_mol_write"] and rec.log[-1][5] == 0 and rec.log[-1][9] == 128 and out[0].shape == (R_, 128)
    assert (rec.log[-1][2], rec.log[-1][4]) == (rec.log[4][11], rec.log[4][12])       # the normal form's words
    rec.log.clear()
    out = M.scaffold_tokens(tok, v, "cpu", generic=True, width=40)
    assert names(rec) == head + ["mdt_mol_scaffold", "mdt_mol_rank", "mdt_mol_write"]
    scaf, rank, write = rec.log[2:5]
    assert scaf[7] == 3 and rank[1:5] == scaf[8:12] == write[1:5] and write[9] == 40         # the scaffold arrays are ranked and written
    assert [tuple(t.shape) for t in out] == [(R_, 40)] + [(R_,)] * 4 and all(t.dtype == torch.int64 for t in out)
    rec.log.clear()
    M.scaffold_tokens(tok, v, "cpu", normalize=True, exocyclic=False)
    assert names(rec) == head + FORM + ["mdt_mol_scaffold", "mdt_mol_rank", "mdt_mol_write"] and rec.log[5][7] == 0
    rec.log.clear()
    out = M.scaffold_keep(tok, v, "cpu")
    assert names(rec) == head + ["mdt_mol_scaffold", "mdt_mol_rank", "mdt_mol_write"]
    graph, scaf, rank, write = rec.log[1:5]
    assert scaf[1:5] == graph[8:12] == rank[1:5] == write[1:5] and scaf[7] == 1             # the MOLECULE is written, not the scaffold
    assert [tuple(t.shape) for t in out] == [(R_, L_), (R_, L_), (R_,), (R_,), (R_,)] and out[1].dtype == torch.bool and not out[1].any()
    rec.log.clear()
    M.scaffold_keep(tok, v, "cpu", normalize=True, exocyclic=False, width=100)
    assert names(rec) == head + FORM + ["mdt_mol_scaffold", "mdt_mol_rank", "mdt_mol_write"] and rec.log[5][7] == 0 and rec.log[-1][9] == 100
    rec.log.clear()
    n, rows = torch.ones(R_, dtype=torch.long), torch.ones(R_, L_, dtype=torch.long)
    out = M.mol_write(n, rows, n, rows, v, "cpu", width=30)
    assert names(rec) == ["mdt_mol_rank", "mdt_mol_write"] and rec.log[1][9] == 30
    assert [tuple(t.shape) for t in out] == [(R_, 30), (R_,), (R_, 30), (R_,)] and all(t.dtype == torch.int64 for t in out)
    rec.log.clear()
    M.mol_write(n.int(), rows.int(), n.int(), rows.int(), v, "cpu", width=128, invariant=False)
    assert names(rec) == ["mdt_mol_write"] and rec.log[0][5] == 0
    rec.log.clear()
    empty = torch.zeros(0, L_, dtype=torch.long)                             # no rows: nothing is launched
    assert M.mol_respell(empty, v, "cpu")[0].shape == (0, L_) and M.scaffold_keep(empty, v, "cpu")[1].shape == (0, L_)
    assert M.scaffold_tokens(empty, v, "cpu", width=7)[0].shape == (0, 7) and rec.log == []


def test_the_public_calls_refuse_before_any_launch(rec):
    tok, v = torch.ones(R_, L_, dtype=torch.long), vocabulary()
    n, rows = torch.ones(R_, dtype=torch.long), torch.ones(R_, L_, dtype=torch.long)
    bad = [lambda: M.mol_respell(tok, v, "cpu", width=129), lambda: M.mol_respell(tok, v, "cpu", width=0), lambda: M.mol_respell(tok, v, "cpu", width=True),
           lambda: M.mol_respell(tok, v, "cpu", invariant=1), lambda: M.mol_respell(tok, v, "cpu", normalize=None),
           lambda: M.mol_respell(torch.ones(R_, 65, dtype=torch.long), v, "cpu"), lambda: M.mol_respell(tok.float(), v, "cpu"),
           lambda: M.mol_respell(tok, None, "cpu"), lambda: M.scaffold_tokens(tok, v, "cpu", generic=1), lambda: M.scaffold_tokens(tok, v, "cpu", width=200),
           lambda: M.scaffold_keep(tok, v, "cpu", exocyclic=0), lambda: M.scaffold_keep(tok, v, "cpu", width=-1),
           lambda: M.scaffold_keep(torch.ones(R_, 65, dtype=torch.long), v, "cpu"),
           lambda: M.mol_write(n, rows, n, rows, v, "cpu", width=None), lambda: M.mol_write(n, rows, n, rows, v, "cpu", width=129),
           lambda: M.mol_write(n, rows.float(), n, rows, v, "cpu", width=8), lambda: M.mol_write(n, rows, n[:3], rows, v, "cpu", width=8),
           lambda: M.mol_write(n, torch.ones(R_, 65, dtype=torch.long), n, torch.ones(R_, 65, dtype=torch.long), v, "cpu", width=8),
           lambda: M.mol_write(n, rows, n, rows, "CNO", "cpu", width=8), lambda: M.mol_write(n, rows, n, rows, v, "cpu", width=8, invariant=None)]
    for call in bad:
        with pytest.raises(ValueError):
            call()
    assert rec.log == []
