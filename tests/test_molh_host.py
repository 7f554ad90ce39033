"""No GPU: the definition of implicit hydrogens and the Kekule check (include/mdt_hip.h, mdt_mol_hydrogens) on its reference
(tests/molh_ref.py) -- the agreed table with hydrogens, verdicts and formulas written by hand, an independent matching oracle
(networkx), invariance under respelling, the step cap -- and the plumbing: C export and argument checks, op schema and shape
inference, the refusals, the launch order of the screening call with ``kekulize`` on a recording library, and the two host helpers
on the formula counts."""
import contextlib
import inspect
import math
import os
import random
import re

import pytest
import torch

import molh_ref as H
import molkey_ref as K
import smiles_ref as S
from conftest import ROOT
import moleculediffusiontransformer_amd as M
from moleculediffusiontransformer_amd import generative as G, ops, runtime as rt

# string -> (hydrogens per atom in order of appearance, formula text with its charge); all written by hand
PLAIN = {
    "CCO": ([3, 2, 1], "C2H6O"), "CC(=O)O": ([3, 0, 0, 1], "C2H4O2"), "CS(C)(=O)=O": ([3, 0, 3, 0, 0], "C2H6O2S"),
    "CS(C)=O": ([3, 0, 3, 0], "C2H6OS"), "C[N+](=O)[O-]": ([3, 0, 0, 0], "CH3NO2"), "[NH4+]": ([4], "H4N+"), "N#N": ([0, 0], "N2"),
    "FC(F)(F)F": ([0, 0, 0, 0, 0], "CF4"), "ClCCl": ([0, 2, 0], "CH2Cl2"), "*C": ([0, 3], "CH3?")}
AROMATIC_OK = {
    "c1ccccc1": ([1] * 6, "C6H6"), "c1ccncc1": ([1, 1, 1, 0, 1, 1], "C5H5N"), "c1cc[nH]c1": ([1] * 5, "C4H5N"),
    "c1ccoc1": ([1, 1, 1, 0, 1], "C4H4O"), "c1ccsc1": ([1, 1, 1, 0, 1], "C4H4S"), "c1cnc[nH]1": ([1, 1, 0, 1, 1], "C3H4N2"),
    "c1ccc2ccccc2c1": ([1, 1, 1, 0, 1, 1, 1, 1, 0, 1], "C10H8"), "c1ccc2[nH]ccc2c1": ([1, 1, 1, 0, 1, 1, 1, 0, 1], "C8H7N"),
    "O=c1cccc[nH]1": ([0, 0, 1, 1, 1, 1, 1], "C5H5NO"),
    "Cn1cnc2c1c(=O)n(C)c(=O)n2C": ([3, 0, 1, 0, 0, 0, 0, 0, 0, 3, 0, 0, 0, 3], "C8H10N4O2"),
    "c1ccc2cccc2cc1": ([1, 1, 1, 0, 1, 1, 1, 0, 1, 1], "C10H8"), "C[n+]1ccccc1": ([3, 0, 1, 1, 1, 1, 1], "C6H8N+"),
    "c1cc[o+]cc1": ([1, 1, 1, 0, 1, 1], "C5H5O+"), "[cH-]1cccc1": ([1] * 5, "C5H5-"), "Cn1cccc1": ([3, 0, 1, 1, 1, 1], "C5H7N"),
    "c1ccn2cccc2c1": ([1, 1, 1, 0, 1, 1, 1, 0, 1], "C8H7N"), "c1ccccc1-c1ccccc1": ([1] * 5 + [0, 0] + [1] * 5, "C12H10"),
    "c1ccccc1c1ccccc1": ([1] * 5 + [0, 0] + [1] * 5, "C12H10")}
NO_KEKULE = {"c1cccc1": ([1] * 5, "C5H5"), "n1cccc1": ([0, 1, 1, 1, 1], "C4H4N"), "c1ccnc1": ([1, 1, 1, 0, 1], "C4H4N"), "c": ([3], "CH3"),
             "cC": ([2, 3], "C2H5"), "c1ccccc1-c": ([1] * 5 + [0, 2], "C7H7")}
OVERVALENT = {"c1cc(C)(C)(C)cc1": (2, [1, 1, 0, 3, 3, 3, 1, 1], "C8H13"), "c1ccc(=C)(C)c1": (3, [1, 1, 1, 0, 2, 3, 1], "C7H9"),
              "o1(C)cccc1": (0, [0, 3, 1, 1, 1, 1], "C5H7O")}
NO_MOLECULE = ["", "C(", "C1CC", "C=C=C=O=C", "c1ccccc", "Xx"]
WEIGHTS = {"C2H6O": 46.069, "C2H4O2": 60.052, "C6H6": 78.114, "C8H10N4O2": 194.194, "H4N+": 18.039, "CH2Cl2": 84.927, "C10H8": 128.174}
TABLE = list(PLAIN) + list(AROMATIC_OK) + list(NO_KEKULE) + list(OVERVALENT)
BACKTRACK = [(0, 1, 5), (0, 2, 5), (1, 2, 5), (1, 3, 5), (3, 4, 5), (3, 5, 5), (4, 5, 5)]
MOST_STEPS = 12                 # 2 x the most the reference makes on the pools below (6; recorded in DESIGN.md)


def atoms_of(s):
    return len(K.graph(s)[2])


@pytest.fixture(scope="module")
def spelled():
    return K.random_spellings()


def respelled_table(rng, spellings=6):
    """-> [(string, [spellings])] for the aromatic rows of the table, written again by molkey_ref.spell from their own graph."""
    out = []
    for s in list(AROMATIC_OK) + list(NO_KEKULE) + list(OVERVALENT):
        _, _, atoms, bonds = K.graph(s)
        g = K.Graph([tok for tok in re.findall(r"\[[^\]]*\]|Cl|Br|[A-Za-z*]", s)], list(bonds))
        assert g.descriptors() == atoms, s
        written = [t for t in (K.spell(g, rng) for _ in range(spellings)) if len(t) <= 64]
        out.append((s, written))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the definition on the reference
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", list(PLAIN) + list(AROMATIC_OK))
def test_agreed_rows_that_pass(s):
    hydrogens, text = {**PLAIN, **AROMATIC_OK}[s]
    r = H.string_hydrogens(s)
    n = atoms_of(s)
    assert (r["verdict"], r["atom"]) == (H.OK, -1) and r["hydrogens"][:n] == hydrogens and not any(r["hydrogens"][n:])
    assert H.formula_string(r["formula"]) == text and r["formula"][0] == sum(hydrogens)


@pytest.mark.parametrize("s", list(NO_KEKULE))
def test_agreed_rows_without_a_kekule_structure(s):
    hydrogens, text = NO_KEKULE[s]
    r = H.string_hydrogens(s)
    assert (r["verdict"], r["atom"]) == (H.NO_KEKULE, -1) and r["hydrogens"][:atoms_of(s)] == hydrogens and not any(r["partner"])
    assert H.formula_string(r["formula"]) == text                            # the formula is written for every verdict


@pytest.mark.parametrize("s", list(OVERVALENT))
def test_agreed_rows_with_an_overvalent_aromatic_atom(s):
    atom, hydrogens, text = OVERVALENT[s]
    r = H.string_hydrogens(s)
    assert (r["verdict"], r["atom"], r["steps"]) == (H.AROMATIC_OVERVALENT, atom, 0)
    assert r["hydrogens"][:atoms_of(s)] == hydrogens and H.formula_string(r["formula"]) == text and not any(r["partner"])


def test_rows_that_are_no_molecule_are_all_zero():
    for s in NO_MOLECULE + [s for s, _ in S.MALFORMED_TABLE + S.OVERVALENT_TABLE]:
        assert s == "" or S.check(s[:64])[0] != 0, s
        r = H.string_hydrogens(s[:64])
        assert (r["verdict"], r["atom"], r["steps"]) == (0, -1, 0) and not any(r["hydrogens"] + r["partner"] + r["formula"]), s
    c = K.descriptor("c")
    for n, nb, bonds in ((3, 1, [(0, 3, 5)]), (9, 0, []), (2, 9, []), (-1, 0, []), (2, -1, []), (0, 0, [])):
        r = H.hydrogens_arrays(n, [c] * 8, nb, bonds, width=8)
        assert r["verdict"] == 0 and r["atom"] == -1 and not any(r["hydrogens"] + r["partner"] + r["formula"])


def test_what_wants_a_double_bond():
    wanting = lambda s: H.string_hydrogens(s)["wanting"]  # noqa: E731
    assert wanting("c1ccccc1") == list(range(6)) and wanting("c1ccncc1") == list(range(6))
    assert wanting("c1cc[nH]c1") == [0, 1, 2, 4] and wanting("[n-]1cccc1") == [1, 2, 3, 4] and wanting("[cH-]1cccc1") == [1, 2, 3, 4]
    assert wanting("Cn1cccc1") == [2, 3, 4, 5] and wanting("c1ccoc1") == [0, 1, 2, 4] and wanting("c1ccsc1") == [0, 1, 2, 4]
    assert wanting("O=c1cccc[nH]1") == [2, 3, 4, 5]                          # neither c(=O) nor [nH]
    assert wanting("C[n+]1ccccc1") == [1, 2, 3, 4, 5, 6] and wanting("c1cc[nH+]cc1") == list(range(6))
    assert wanting("c1cc[o+]cc1") == list(range(6)) and wanting("c1cc[s+]cc1") == list(range(6))
    assert wanting("[Si](C)(C)C") == [] and wanting("C=C") == []
    # an explicit '-' between two rings is no edge, a bare cc bond is one; cc is kekulisable as ethene (rings are not checked)
    assert (5, 6) not in H.string_hydrogens("c1ccccc1-c1ccccc1")["edges"] and (5, 6) in H.string_hydrogens("c1ccccc1c1ccccc1")["edges"]
    assert [H.string_hydrogens(s)["verdict"] for s in ("cc", "c:c", "c-c", "c=c")] == [0, 0, 2, 2]
    assert H.string_hydrogens("cc")["hydrogens"][:2] == [2, 2] and H.string_hydrogens("cc")["partner"][:2] == [2, 1]


def test_entries_that_no_scan_writes():
    c, f = K.descriptor("c"), K.descriptor("F") | 1 << 10
    twice = H.hydrogens_arrays(2, [c, c], 2, [(0, 1, 5)] * 2, width=8)       # an entry listed twice counts twice in the sum
    assert twice["hydrogens"][:2] == [1, 1] and twice["verdict"] == 0 and twice["partner"][:2] == [2, 1]
    loop = H.hydrogens_arrays(2, [c, c], 2, [(0, 0, 5), (0, 1, 5)], width=8)  # (a, a): twice at a, never an edge
    assert loop["hydrogens"][:2] == [0, 2] and loop["edges"] == [(0, 1)] and loop["verdict"] == 0
    alone = H.hydrogens_arrays(1, [c], 1, [(0, 0, 5)], width=1)
    assert alone["hydrogens"] == [1] and alone["wanting"] == [0] and alone["verdict"] == H.NO_KEKULE
    odd = H.hydrogens_arrays(3, [c] * 3, 2, [(0, 1, 5), (2, 1, 5)], width=8)
    assert odd["verdict"] == H.NO_KEKULE and odd["steps"] == 0 and odd["wanting"] == [0, 1, 2]
    fluor = H.hydrogens_arrays(2, [c, f], 1, [(0, 1, 5)], width=8)           # a lower-case symbol without a list
    assert (fluor["verdict"], fluor["atom"]) == (H.AROMATIC_OVERVALENT, 1)
    big = H.hydrogens_arrays(2, [K.descriptor("C")] * 2, 1, [(0, 1, 65535)], width=8)
    assert big["verdict"] == 0 and big["hydrogens"][:2] == [0, 0]


def pools(spelled):
    rng = random.Random(3)
    rows = [s for _, sp in spelled for s in sp] + TABLE + [t for _, sp in respelled_table(rng) for t in sp]
    return rows + [s[:64] for s in S.mutated_rows(512)]


def test_verdict_zero_means_a_perfect_matching_exists(spelled):
    """The independent oracle: on the wanting subgraph, networkx's maximum-cardinality matching is perfect exactly when the
    reference's search says 0; and on 0 the partners are a perfect matching of W over the edges."""
    import networkx as nx
    decided = searched = 0
    for s in pools(spelled):
        r = H.string_hydrogens(s)
        if r["verdict"] not in (H.OK, H.NO_KEKULE):
            continue
        g = nx.Graph()
        g.add_nodes_from(r["wanting"])
        g.add_edges_from(r["edges"])
        perfect = 2 * len(nx.max_weight_matching(g, maxcardinality=True)) == len(r["wanting"])
        assert perfect == (r["verdict"] == H.OK), s
        decided += 1
        searched += bool(r["wanting"])
        pairs = {a: p - 1 for a, p in enumerate(r["partner"]) if p}
        if r["verdict"] == H.OK:
            assert sorted(pairs) == r["wanting"] and all(pairs[b] == a and (min(a, b), max(a, b)) in r["edges"] for a, b in pairs.items()), s
        else:
            assert not pairs
    assert decided > 2500 and searched > 400


def test_spelling_invariance(spelled):
    def seen(s):
        r = H.string_hydrogens(s)
        atoms = K.graph(s)[2]
        return r["verdict"], tuple(r["formula"]), sorted(zip(atoms, r["hydrogens"]))
    asked = 0
    for g, sp in list(spelled) + respelled_table(random.Random(4)):
        first = seen(sp[0])
        assert first[2] or isinstance(g, str)
        for t in sp[1:]:
            assert seen(t) == first, (sp[0], t)
            asked += 1
    assert asked > 1500
    for s, sp in respelled_table(random.Random(4)):                          # ... and equal to the row as the table writes it
        assert all(seen(t) == seen(s) for t in sp), s


def test_no_row_of_the_pools_is_undecided_and_the_steps_stay_small(spelled):
    """The condition on the pools: nothing is UNDECIDED at 4096, and the most steps a row takes (6: one try per pair of a biphenyl,
    none taken back) stays under twice what the reference was measured to make."""
    results = [H.string_hydrogens(s) for s in pools(spelled)]
    worst = max(r["steps"] for r in results)
    print("most steps of a row: %d; verdicts %s" % (worst, [sum(r["verdict"] == v for r in results) for v in range(4)]))
    assert not any(r["verdict"] == H.UNDECIDED for r in results) and H.MAX_STEPS == 4096
    assert worst <= MOST_STEPS and worst * 2 >= MOST_STEPS


def test_max_steps_is_honoured():
    for s, full in (("c1ccc2ccccc2c1", 5), ("c1ccc2cccc2cc1", 5)):
        assert H.string_hydrogens(s)["steps"] == full
        for cap in (1, 2, 3):
            r = H.string_hydrogens(s, cap=cap)
            assert (r["verdict"], r["steps"]) == (H.UNDECIDED, cap) and not any(r["partner"]), (s, cap)
        assert H.string_hydrogens(s, cap=full)["verdict"] == H.OK
    assert H.string_hydrogens("c1ccccc1", cap=3)["verdict"] == H.OK and H.string_hydrogens("c1ccccc1", cap=2)["verdict"] == H.UNDECIDED
    assert H.string_hydrogens("c1cccc1", cap=1)["verdict"] == H.NO_KEKULE    # |W| odd: decided in zero steps under any cap
    assert H.string_hydrogens("CCO", cap=1)["verdict"] == H.OK


def test_a_try_is_taken_back_where_the_first_choice_fails():
    """A graph on which the pick's first candidate leaves an atom alone: the search goes back, and the count says so."""
    c = K.descriptor("c")
    # two triangles 0 1 2 and 3 4 5 joined by 1 - 3: atom 0 is picked first (two neighbours, lowest index) and tries 1 first,
    # which leaves 2 alone; the try is taken back and 0 - 2, 1 - 3, 4 - 5 follow: four steps for three pairs
    r = H.hydrogens_arrays(6, [c] * 6, 7, BACKTRACK, width=8)
    assert r["verdict"] == H.OK and r["partner"][:6] == [3, 4, 1, 2, 6, 5] and r["steps"] == 4
    assert H.hydrogens_arrays(6, [c] * 6, 7, BACKTRACK, width=8, cap=3)["verdict"] == H.UNDECIDED
    star = H.hydrogens_arrays(4, [c] * 4, 3, [(0, 1, 5), (0, 2, 5), (0, 3, 5)], width=8)   # three leaves want one centre
    assert star["verdict"] == H.NO_KEKULE and star["steps"] == 1
    ring8 = H.hydrogens_arrays(8, [c] * 8, 8, [(i, (i + 1) % 8, 5) for i in range(8)], width=8)
    assert ring8["verdict"] == H.OK and ring8["steps"] == 4


# ---------------------------------------------------------------------------------------------------------------------
# header, library, binding
# ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_the_library_exports_the_new_symbol():
    hdr = open(os.path.join(ROOT, "include", "mdt_hip.h")).read()
    lib = rt.load_library()
    assert re.search(r"\bint mdt_mol_hydrogens\s*\(", hdr) and "mdt_mol_hydrogens" in rt.SYMBOLS and hasattr(lib, "mdt_mol_hydrogens")
    assert len(rt.SYMBOLS["mdt_mol_hydrogens"][1]) == 13
    assert int(re.search(r"#define MDT_ABI_VERSION (\d+)", hdr).group(1)) == rt.ABI_VERSION == 5 == lib.mdt_abi_version()
    assert int(re.search(r"#define MDT_MOLH_MAX_STEPS (\d+)", hdr).group(1)) == rt.MOLH_MAX_STEPS == G.MOLH_MAX_STEPS == H.MAX_STEPS
    assert int(re.search(r"#define MDT_MOLH_FORMULA (\d+)", hdr).group(1)) == rt.MOLH_FORMULA == len(G.FORMULA_SLOTS) == len(H.SLOTS)
    for name, value in (("OK", 0), ("AROMATIC_OVERVALENT", 1), ("NO_KEKULE", 2), ("UNDECIDED", 3)):
        assert int(re.search(r"MDT_MOLH_%s = (\d+)" % name, hdr).group(1)) == getattr(rt, "MOLH_" + name) == getattr(H, name) == value
    assert G.FORMULA_SLOTS == H.SLOTS and rt.SCREEN_OVERVALENT == H.OVERVALENT_BIT == 64
    flat = " ".join(hdr.replace(" * ", " ").split())
    for phrase in ("not RDKit's sanitisation", "Ring membership is not checked", "cc is kekulisable as ethene", "No radicals",
                   "Bracket atoms are taken at their word", "a definition, not a measurement", "ITS ORDER IS PART OF THE DEFINITION"):
        assert phrase in flat, phrase
    assert "k_molh.hip" in [s for s, _ in __import__("moleculediffusiontransformer_amd.build", fromlist=["SOURCES"]).SOURCES]
    src = open(os.path.join(ROOT, "moleculediffusiontransformer_amd", "csrc", "k_molh.hip")).read()
    assert "molh_atom(" in src and "molh_slot(" in src and "mdt_molh.h" in src   # the kernel applies the rule the host check runs


def test_entry_point_refuses_bad_arguments_before_any_launch():
    lib = rt.load_library()

    def call(L=32, R_=5, steps=4096, p=8, out=8):
        return lib.mdt_mol_hydrogens(p, p, p, p, L, R_, steps, out, out, out, out, out, 0)
    for kw, what in ((dict(L=0), b"L <= 64"), (dict(L=65), b"L <= 64"), (dict(R_=-1), b"R >= 0"), (dict(steps=0), b"max_steps <= 4096"),
                     (dict(steps=4097), b"max_steps <= 4096"), (dict(p=0), b"null"), (dict(out=0), b"null")):
        assert call(**kw) == 2, kw
        assert what in lib.mdt_last_error(), (kw, lib.mdt_last_error())
    assert call(R_=0) == 0 and call(R_=0, p=0, out=0) == 0                   # nothing to do: nothing is launched, nothing is read
    assert call(R_=0, steps=1) == 0 and call(R_=0, steps=0) != 0 and call(R_=0, L=65) != 0


def vocabulary():
    return M.SmilesVocabulary([None] + S.CHARS)


def test_op_schema_and_shape_inference():
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert str(torch.ops.mdt.mol_hydrogens.default._schema) == \
        "mdt::mol_hydrogens(Tensor natoms, Tensor atoms, Tensor nbonds, Tensor bonds, SymInt max_steps) -> (Tensor, Tensor, Tensor, Tensor, Tensor)"
    with FakeTensorMode():
        n, rows = torch.empty(15, dtype=torch.int32), torch.empty(15, 40, dtype=torch.int32)
        out = torch.ops.mdt.mol_hydrogens(n, rows, n, rows, 4096)
        assert [(tuple(t.shape), t.dtype) for t in out] == [((15, 40), torch.uint8), ((15, 40), torch.uint8), ((15,), torch.uint8),
                                                            ((15,), torch.int32), ((15, 13), torch.int32)]
    n, rows = torch.zeros(3, dtype=torch.int32), torch.zeros(3, 4, dtype=torch.int32)       # no CPU implementation behind the op
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        torch.ops.mdt.mol_hydrogens(n, rows, n, rows, 1)


# ---------------------------------------------------------------------------------------------------------------------
# on a recording library: launch order, refusals with nothing launched
# ---------------------------------------------------------------------------------------------------------------------
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


class Fwd:
    max_length = 24

    def __init__(self, rec):
        self.rec = rec

    def sample(self, data, device, **k):
        self.rec.log.append(("forward_sample", data, k))
        return torch.zeros(data.shape[0], 1, 24)


N_, G_, K_, L_, n_ = 5, 3, 2, 16, 12


def names(rec):
    return [e[0] for e in rec.log]


def test_launch_order_of_the_screening_call_with_and_without_kekulize(rec):
    tok, cond, v = torch.ones(N_ * G_, L_, dtype=torch.long), torch.zeros(G_, n_), vocabulary()
    known = M.KnownSet(torch.ones(4, L_, dtype=torch.long), L_)
    need, bad = M.SubstructureSet(["C=O", "N"], v), M.SubstructureSet(["C#N", "OO", "c1ccccc1"], v)
    need.on("cpu"), bad.on("cpu")                                            # (the patterns' graphs: once per device, not here)
    run = lambda **kw: (rec.log.clear(), M.screen_tokens_diverse(Fwd(rec), tok, cond, "cpu", N_, K_, **kw), names(rec)[3:])[2]  # noqa: E731
    # every combination the substructure test lists: kekulize=False makes the launches made without the keyword ...
    parent = [
        (dict(), ["mdt_screen_select"]),
        (dict(vocabulary=v), ["mdt_smiles_check", "mdt_screen_select_reject"]),
        (dict(min_distance=2), ["mdt_screen_select_diverse"]),
        (dict(vocabulary=v, min_distance=2), ["mdt_smiles_check", "mdt_screen_select_diverse_reject"]),
        (dict(known_tokens=known, min_novelty=2), ["mdt_edit_nearest", "mdt_screen_select_diverse"]),
        (dict(vocabulary=v, identity="graph"), ["mdt_smiles_check", "mdt_mol_graph", "mdt_mol_key", "mdt_key_flags", "mdt_screen_select_reject"]),
        (dict(vocabulary=v, max_similarity=0.5), ["mdt_smiles_check", "mdt_mol_graph", "mdt_mol_fp", "mdt_screen_select_similar"]),
        (dict(vocabulary=v, require=need), ["mdt_smiles_check", "mdt_mol_graph", "mdt_sub_match", "mdt_screen_select_reject"]),
        (dict(vocabulary=v, forbid=bad), ["mdt_smiles_check", "mdt_mol_graph", "mdt_sub_match", "mdt_screen_select_reject"]),
        (dict(vocabulary=v, require=need, forbid=bad), ["mdt_smiles_check", "mdt_mol_graph", "mdt_sub_match", "mdt_screen_select_reject"]),
        (dict(vocabulary=v, identity="graph", require=need, forbid=bad, max_similarity=0.5),
         ["mdt_smiles_check", "mdt_mol_graph", "mdt_mol_key", "mdt_key_flags", "mdt_sub_match", "mdt_mol_fp", "mdt_screen_select_similar"]),
        (dict(vocabulary=v, known_tokens=known, identity="graph", forbid=bad, max_known_similarity=0.7, min_novelty=2),
         ["mdt_smiles_check", "mdt_mol_graph", "mdt_mol_key", "mdt_key_flags", "mdt_sub_match", "mdt_mol_fp", "mdt_fp_nearest",
          "mdt_edit_nearest", "mdt_screen_select_diverse_reject"])]
    known.mol_keys(v, "cpu"), known.fingerprints(v, "cpu")                   # (the known set's keys and fingerprints: once)
    for kw, want in parent:
        logs = []
        for extra in (dict(), dict(kekulize=False)):
            assert run(**kw, **extra) == want, kw
            logs.append([(e[0], len(e), tuple(a for a in e[1:] if isinstance(a, int) and a < 4096)) for e in rec.log])
        assert logs[0] == logs[1]
        if "vocabulary" not in kw:
            continue
        # ... and kekulize=True adds exactly one mdt_mol_hydrogens, right after the one mdt_mol_graph over the candidates
        got = run(**kw, kekulize=True)
        if "mdt_mol_graph" in want:
            at = want.index("mdt_mol_graph") + 1
            assert got == want[:at] + ["mdt_mol_hydrogens"] + want[at:], kw
        else:
            assert got == [want[0], "mdt_mol_graph", "mdt_mol_hydrogens"] + [w if w.endswith("reject") else w + "_reject" for w in want[1:]], kw
        graph = rec.log[3 + got.index("mdt_mol_graph")]
        molh = rec.log[3 + got.index("mdt_mol_hydrogens")]
        assert molh[1:5] == graph[8:12] and molh[5:8] == (L_, N_ * G_, 4096) and len(molh) == 1 + 13 and 0 not in molh[8:13]
        for e in rec.log:                                                    # the one graph feeds every consumer
            if e[0] in ("mdt_mol_key", "mdt_sub_match", "mdt_mol_fp"):
                assert e[1:5] == graph[8:12]
    # the public calls
    rec.log.clear()
    out = M.mol_hydrogens(tok.to(torch.int16), v, "cpu", max_steps=7)
    assert names(rec) == ["mdt_tokens_compact", "mdt_mol_graph", "mdt_mol_hydrogens"] and rec.log[2][5:8] == (L_, N_ * G_, 7)
    assert [tuple(t.shape) for t in out] == [(N_ * G_, L_)] * 2 + [(N_ * G_,)] * 4 and all(t.dtype == torch.int64 for t in out)
    rec.log.clear()
    counts, verdict, status, position = M.mol_formula(tok, v, "cpu")
    assert names(rec) == ["mdt_tokens_compact", "mdt_mol_graph", "mdt_mol_hydrogens"] and rec.log[2][7] == 4096
    assert counts.shape == (N_ * G_, 13) and all(t.dtype == torch.int64 and t.shape == (N_ * G_,) for t in (verdict, status, position))


def test_screen_candidates_forwards_kekulize_only_when_set(rec, monkeypatch):
    seen = {}

    class Inv:
        max_length = 32

        def sample_tokens(self, seq, device, **k):
            return torch.ones(seq.shape[0], 32, dtype=torch.long)
    monkeypatch.setattr(G, "screen_tokens", lambda *a, **k: seen.update(plain=k) or "plain")
    monkeypatch.setattr(G, "screen_tokens_diverse", lambda *a, **k: seen.update(diverse=k) or "diverse")
    cond, v = torch.zeros(2, 12), vocabulary()
    assert M.screen_candidates(Inv(), "fwd", cond, "dev", 3, 2, vocabulary=v, kekulize=True) == "diverse"
    assert seen["diverse"] == dict(min_distance=1, min_novelty=1, vocabulary=v, kekulize=True)
    assert M.screen_candidates(Inv(), "fwd", cond, "dev", 3, 2, vocabulary=v, kekulize=False) == "diverse"
    assert seen["diverse"] == dict(min_distance=1, min_novelty=1, vocabulary=v)
    assert M.screen_candidates(Inv(), "fwd", cond, "dev", 3, 2, kekulize=False) == "plain" and seen["plain"] == dict()
    assert rec.log == []


def test_refusals_come_before_anything_is_launched(rec):
    fwd, v = Fwd(rec), vocabulary()
    tok, cond = torch.ones(N_ * G_, L_, dtype=torch.long), torch.zeros(G_, n_)
    wide = torch.ones(N_ * G_, 65, dtype=torch.long)
    div = lambda t=tok, **kw: M.screen_tokens_diverse(fwd, t, cond, "cpu", N_, K_, **kw)  # noqa: E731

    class Inv:
        max_length = 65

        def sample_tokens(self, *a, **k):
            raise AssertionError("sampled")
    for call, what in (
            (lambda: div(kekulize=True), "give a vocabulary"),
            (lambda: div(wide, vocabulary=v, kekulize=True), "at most 64"),
            (lambda: div(vocabulary=v, kekulize=1), "True or False"),
            (lambda: div(vocabulary=v, kekulize=None), "True or False"),
            (lambda: M.screen_candidates(Inv(), fwd, cond, "cpu", N_, K_, vocabulary=v, kekulize=True), "at most 64"),
            (lambda: M.screen_candidates(Inv(), fwd, cond, "cpu", N_, K_, kekulize=True), "give a vocabulary"),
            (lambda: M.mol_hydrogens(wide, v, "cpu"), "at most 64"),
            (lambda: M.mol_hydrogens(tok.float(), v, "cpu"), "integer"),
            (lambda: M.mol_hydrogens(tok, S.CHARS, "cpu"), "SmilesVocabulary"),
            (lambda: M.mol_hydrogens(tok[:, :0], v, "cpu"), "at least one position"),
            (lambda: M.mol_hydrogens(tok, v, "cpu", max_steps=0), r"\[1, 4096\]"),
            (lambda: M.mol_hydrogens(tok, v, "cpu", max_steps=4097), r"\[1, 4096\]"),
            (lambda: M.mol_hydrogens(tok, v, "cpu", max_steps=2.0), r"\[1, 4096\]"),
            (lambda: M.mol_formula(wide, v, "cpu"), "at most 64"),
            (lambda: M.mol_formula(tok, None, "cpu"), "SmilesVocabulary"),
            (lambda: M.formula_strings(torch.zeros(2, 12, dtype=torch.long)), r"\(R, 13\)"),
            (lambda: M.mol_weight(torch.zeros(2, 13)), r"\(R, 13\)")):
        with pytest.raises(ValueError, match=what):
            call()
    assert rec.log == []
    with pytest.raises(TypeError):                                           # screen_tokens keeps its parameter list
        M.screen_tokens(fwd, tok, cond, "cpu", N_, K_, kekulize=True)
    # the op refuses what the kernel does not take
    n, rows = torch.zeros(3, dtype=torch.int32), torch.zeros(3, 8, dtype=torch.int32)
    molh = torch.ops.mdt.mol_hydrogens
    for call, what in ((lambda: molh(n, torch.zeros(3, 65, dtype=torch.int32), n, torch.zeros(3, 65, dtype=torch.int32), 1), "1 to 64"),
                       (lambda: molh(n, torch.zeros(3, 0, dtype=torch.int32), n, torch.zeros(3, 0, dtype=torch.int32), 1), "1 to 64"),
                       (lambda: molh(n, rows.long(), n, rows, 1), "int32"), (lambda: molh(n.long(), rows, n, rows, 1), "int32"),
                       (lambda: molh(n, rows, n, rows[:, :4], 1), "int32"), (lambda: molh(n[:2], rows, n, rows, 1), "one value per row"),
                       (lambda: molh(n, rows, n, rows, 0), r"\[1, 4096\]"), (lambda: molh(n, rows, n, rows, 4097), r"\[1, 4096\]")):
        with pytest.raises(RuntimeError, match=what):
            call()
    assert rec.log == []


# ---------------------------------------------------------------------------------------------------------------------
# the host helpers on the counts, and the public surface
# ---------------------------------------------------------------------------------------------------------------------
def test_formula_strings_and_mol_weight_on_the_table():
    table = {**PLAIN, **AROMATIC_OK, **NO_KEKULE}
    strings = list(table) + ["", "C(", "[2H]O[2H]", "[Ca+2]", "[O-]C(=O)C([O-])=O", "BrCI", "B(F)(F)F", "OP(O)(O)=O"]
    counts = torch.tensor([H.string_hydrogens(s)["formula"] for s in strings])
    texts = M.formula_strings(counts)
    assert texts[:len(table)] == [text for _, text in table.values()]
    assert texts[len(table):] == ["", "", "H2O", "+2?", "C2O4-2", "CH2BrI", "BF3", "H3O4P"]
    assert texts == [H.formula_string(row) for row in counts.tolist()] == M.formula_strings(counts.int().numpy())
    weight = M.mol_weight(counts)
    assert weight.dtype == torch.float64 and weight.shape == (len(strings),)
    for s, w in zip(strings, weight.tolist()):
        want = H.weight(H.string_hydrogens(s)["formula"])
        assert (math.isnan(w) and math.isnan(want)) or abs(w - want) < 1e-9, s
        text = H.formula_string(H.string_hydrogens(s)["formula"])
        if text in WEIGHTS:
            assert abs(w - WEIGHTS[text]) < 2e-3, s                          # the handbook's value
    by = dict(zip(strings, weight.tolist()))
    assert math.isnan(by["*C"]) and math.isnan(by["[Ca+2]"]) and by[""] == 0.0 and by["C("] == 0.0
    assert M.formula_strings(torch.zeros(0, 13, dtype=torch.long)) == [] and M.mol_weight(torch.zeros(0, 13, dtype=torch.long)).shape == (0,)


def test_public_surface_and_what_the_docstrings_promise():
    for name in ("mol_hydrogens", "mol_formula", "formula_strings", "mol_weight"):
        assert getattr(M, name) is getattr(G, name)
    p = inspect.signature(M.screen_tokens_diverse).parameters
    assert p["kekulize"].default is False and list(p)[-1] == "screen_tokens_kwargs" and "kekulize" not in inspect.signature(M.screen_tokens).parameters
    assert list(inspect.signature(M.mol_hydrogens).parameters) == ["tokens", "vocabulary", "device", "max_steps"]
    assert inspect.signature(M.mol_hydrogens).parameters["max_steps"].default == 4096
    assert list(inspect.signature(M.mol_formula).parameters) == ["tokens", "vocabulary", "device"]
    flat = " ".join(M.mol_hydrogens.__doc__.split())
    for phrase in ("not RDKit's sanitisation", "Ring membership is not checked", "no radicals", "bracket atoms are taken at their word",
                   "can depend on how the row is spelled", "4096"):
        assert phrase in flat, phrase
    flat = " ".join(M.screen_tokens_diverse.__doc__.split())
    for phrase in ("No status bit is free", "bit 64 also means", "undecided after 4096 steps, which counts against the row",
                   "exactly the launches it makes without the keyword"):
        assert phrase in flat, phrase
