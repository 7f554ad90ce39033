"""No GPU: the definition of the graph key (include/mdt_hip.h, mdt_mol_graph / mdt_mol_key) on its string-level reference
(tests/molkey_ref.py) -- invariance under respelling, the agreed equal and unequal pairs, discrimination against networkx's
isomorphism test, key 0 -- and the plumbing: C exports and argument checks, op schemas and shape inference, the refusals, and the
launch order of the screening calls with ``identity=`` on a recording library."""
import contextlib
import os
import re

import numpy as np
import pytest
import torch

import molkey_ref as K
import smiles_ref as S
from conftest import ROOT
import moleculediffusiontransformer_amd as M
from moleculediffusiontransformer_amd import generative as G, ops, runtime as rt

EQUAL, DIFFERENT = K.EQUAL_PAIRS, K.DIFFERENT_PAIRS


@pytest.fixture(scope="module")
def spelled():
    return K.random_spellings()


# ---------------------------------------------------------------------------------------------------------------------
# the definition on the reference
# ---------------------------------------------------------------------------------------------------------------------
def test_every_spelling_is_a_molecule_and_all_spellings_of_a_graph_give_one_key(spelled):
    assert len(spelled) == 500 and all(len(sp) == 4 for _, sp in spelled)
    assert sum(len(set(sp)) > 1 for _, sp in spelled) >= 350                 # the writer does respell
    assert max(len(g.atoms) for g, _ in spelled) == 20 and max(len(s) for _, sp in spelled for s in sp) <= K.MAX_TOKENS
    text = "".join(s for _, sp in spelled for s in sp)
    for needle in ("%", "[NH4+]", "[O-]", "c", ".", "-", ":", "=", "#", "(", "[nH]"):
        assert needle in text, needle
    for g, sp in spelled:
        for s in sp:
            assert S.check(s) == (S.OK, -1), (s, g.atoms, g.bonds)           # no test below can pass on rows that all get key 0
        keys = {K.string_key(s) for s in sp} | {K.key(g.descriptors(), g.bonds)}
        assert len(keys) == 1 and 0 not in keys, (sp, keys)
        _, _, atoms, bonds = K.graph(sp[0])
        assert sorted(atoms) == sorted(g.descriptors()) and len(bonds) == len(g.bonds)


@pytest.mark.parametrize("a,b", EQUAL)
def test_pairs_that_must_be_equal(a, b):
    assert S.check(a) == S.check(b) == (S.OK, -1)
    assert K.string_key(a) == K.string_key(b) != 0


@pytest.mark.parametrize("a,b", DIFFERENT)
def test_pairs_that_must_differ(a, b):
    assert S.check(a) == S.check(b) == (S.OK, -1)
    assert K.string_key(a) != K.string_key(b) and K.string_key(a) and K.string_key(b)


def test_the_rooting_is_what_separates_three_of_the_pairs():
    for a, b in DIFFERENT[3:6]:
        plain = [K.key(*K.graph(s)[2:], rooted=False) for s in (a, b)]
        assert plain[0] == plain[1], (a, b)                                  # the unrooted form of the same hash cannot tell them apart


def test_graph_of_a_row_descriptors_and_bond_orders():
    d = K.descriptor
    assert K.graph("CCO")[2:] == ([d("C"), d("C"), d("O")], [(0, 1, 1), (1, 2, 1)])
    assert K.graph("ClC(Br)=O")[2:] == ([d("Cl"), d("C"), d("Br"), d("O")], [(0, 1, 1), (1, 2, 1), (1, 3, 2)])
    assert d("C") == 2 | 9 << 12 and d("Cl") == 2 | 12 << 5 | 9 << 12 and d("c") == 2 | 1 << 10 | 9 << 12 and d("*") == 26 | 9 << 12
    assert K.graph("[13CH4]")[2] == [2 | 1 << 11 | 9 << 12 | 4 << 17 | 13 << 21]
    assert K.graph("[NH4+]")[2] == [13 | 1 << 11 | 10 << 12 | 4 << 17] and K.graph("[O-]C")[2][0] == 14 | 1 << 11 | 8 << 12
    assert K.graph("[Fe++]")[2] == K.graph("[Fe+2]")[2] == [5 | 5 << 5 | 1 << 11 | 11 << 12]
    assert K.graph("[C@@H](N)(O)C")[2][0] == K.graph("[CH:7]")[2][0] == 2 | 1 << 11 | 9 << 12 | 1 << 17      # chirality, class: ignored
    assert K.graph("[nH]1cccc1")[2][0] == 13 | 1 << 10 | 1 << 11 | 9 << 12 | 1 << 17
    assert K.graph("[2049C]")[2] == K.graph("[1C]")[2]                       # the isotope is kept modulo 2048
    # no symbol: 5 between two aromatic atoms, else 1; a closure takes whichever end's symbol is present
    assert [o for _, _, o in K.graph("c1ccccc1C")[3]] == [5, 5, 5, 5, 5, 5, 1]
    assert K.graph("c1ccccc1-c1ccccc1")[3][6] == (5, 6, 1) and K.graph("C:C")[3] == [(0, 1, 5)]
    assert K.graph("C=1CC1")[3] == K.graph("C1CC=1")[3] == K.graph("C=1CC=1")[3] == [(0, 1, 1), (1, 2, 1), (0, 2, 2)]
    assert K.graph("C$C")[3] == [(0, 1, 4)] and K.graph("CC#N")[3] == [(0, 1, 1), (1, 2, 3)] and K.graph("C/C=C\\C")[3] == [(0, 1, 1), (1, 2, 2), (2, 3, 1)]
    assert K.graph("C(C)(N)O")[3] == [(0, 1, 1), (0, 2, 1), (0, 3, 1)] and K.graph("C.C")[3] == [] and K.graph("C1.C1")[3] == [(0, 1, 1)]
    # these count as different molecules, and stereo is ignored
    assert K.string_key("[CH4]") != K.string_key("C") and K.string_key("[C]") != K.string_key("C")
    assert K.string_key("C[C@H](N)O") == K.string_key("C[C@@H](N)O") == K.string_key("C[CH](N)O")


def test_key_zero_means_no_molecule():
    assert K.string_key("") == 0 and K.graph("")[:2] == (S.OK, -1)
    for s, _ in S.MALFORMED_TABLE + S.OVERVALENT_TABLE:
        assert K.string_key(s) == 0 and K.graph(s)[2:] == ([], []), s
    assert all(K.string_key(s) != 0 for s in S.OK_TABLE)
    assert K.mix(0) == 0xE220A8397B1DCDAF                                    # splitmix64's first output for seed 0


def to_networkx(descriptors, bonds):
    import networkx as nx
    g = nx.Graph()
    g.add_nodes_from((i, {"d": d}) for i, d in enumerate(descriptors))
    g.add_edges_from((a, b, {"o": o}) for a, b, o in bonds)
    return g


def test_distinct_keys_for_every_small_graph():
    nx = pytest.importorskip("networkx")
    atlas = [g for g in nx.graph_atlas_g() if len(g) >= 1 and max(dict(g.degree).values()) <= 4]
    assert len(atlas) == 684                                                 # at most 7 nodes, degree at most 4, disconnected ones included
    carbon = K.descriptor("C")
    keys = {}
    for i, g in enumerate(atlas):
        nodes = {v: j for j, v in enumerate(g.nodes)}
        k = K.key([carbon] * len(g), [(nodes[a], nodes[b], 1) for a, b in g.edges])
        assert k != 0 and k not in keys, (i, keys.get(k))
        keys[k] = i


def test_equal_keys_exactly_where_the_graphs_are_isomorphic(spelled):
    nx = pytest.importorskip("networkx")
    from networkx.algorithms.isomorphism import categorical_edge_match, categorical_node_match
    graphs = [(K.string_key(sp[0]), to_networkx(g.descriptors(), g.bonds)) for g, sp in spelled]

    def same(a, b):
        return nx.is_isomorphic(a, b, node_match=categorical_node_match("d", None), edge_match=categorical_edge_match("o", None))

    def coarse(g):                                                           # equal for isomorphic graphs: only such pairs are looked at
        return (tuple(sorted(d for _, d in g.nodes(data="d"))), tuple(sorted(o for _, _, o in g.edges(data="o"))),
                tuple(sorted(dict(g.degree).values())))
    by_coarse = {}
    for k, g in graphs:
        by_coarse.setdefault(coarse(g), []).append((k, g))
    compared = 0
    for group in by_coarse.values():
        for i, (ka, a) in enumerate(group):
            for kb, b in group[:i]:
                compared += 1
                assert (ka == kb) == same(a, b), (ka, kb, a.nodes(data=True), a.edges(data=True), b.edges(data=True))
    assert compared >= 100
    keys = {}
    for k, g in graphs:                                                      # and no two coarse classes share a key
        assert keys.setdefault(k, coarse(g)) == coarse(g)


# ---------------------------------------------------------------------------------------------------------------------
# header, library, binding
# ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_the_library_exports_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "mdt_hip.h")).read()
    lib = rt.load_library()
    for name, arity in (("mdt_mol_graph", 14), ("mdt_mol_key", 8), ("mdt_key_flags", 7)):
        assert re.search(r"\bint %s\s*\(" % name, hdr) and name in rt.SYMBOLS and hasattr(lib, name), name
        assert len(rt.SYMBOLS[name][1]) == arity
    assert int(re.search(r"#define MDT_ABI_VERSION (\d+)", hdr).group(1)) == rt.ABI_VERSION == 5 == lib.mdt_abi_version()
    for phrase in ("0xA5A5A5A5A5A5A5A5", "0x100000001B3", "KEY 0 MEANS", "refinement hash, not a", "isotope number modulo 2048",
                   "[CH4] and C differ", "stereo is ignored"):
        assert phrase in hdr, phrase
    assert "k_molgraph.hip" in [s for s, _ in __import__("moleculediffusiontransformer_amd.build", fromlist=["SOURCES"]).SOURCES]


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = rt.load_library()

    def graph(L=32, R_=5, p=8, out=8):
        return lib.mdt_mol_graph(p, p, L, R_, p, p, p, out, out, out, out, out, out, 0)

    def key(L=32, R_=5, p=8):
        return lib.mdt_mol_key(p, p, p, p, L, R_, p, 0)

    def flags(N=4, G_=3, M_=0, p=8, known=0):
        return lib.mdt_key_flags(p, N, G_, known, M_, p, 0)
    for call, kw, what in ((graph, dict(L=0), b"L <= 64"), (graph, dict(L=65), b"L <= 64"), (graph, dict(R_=-1), b"R >= 0"),
                           (graph, dict(p=0), b"null"), (graph, dict(out=0), b"null"),
                           (key, dict(L=0), b"L <= 64"), (key, dict(L=65), b"L <= 64"), (key, dict(R_=-1), b"R >= 0"), (key, dict(p=0), b"null"),
                           (flags, dict(N=0), b"N <= 1024"), (flags, dict(N=1025), b"N <= 1024"), (flags, dict(p=0), b"null"),
                           (flags, dict(M_=3), b"null"), (flags, dict(M_=-1), b"M >= 0"), (flags, dict(G_=-1), b"G >= 0")):
        assert call(**kw) != 0, (call.__name__, kw)
        assert what in lib.mdt_last_error(), (call.__name__, kw, lib.mdt_last_error())
    # nothing to do: nothing is launched, nothing is read
    assert graph(R_=0) == 0 and graph(R_=0, p=0, out=0) == 0 and key(R_=0) == 0 and key(R_=0, p=0) == 0
    assert flags(G_=0) == 0 and flags(G_=0, p=0) == 0


def vocabulary():
    return M.SmilesVocabulary([None] + S.CHARS)


def test_ops_schema_and_shape_inference():
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert str(torch.ops.mdt.mol_graph.default._schema) == \
        ("mdt::mol_graph(Tensor packed, Tensor length, Tensor classes, Tensor max_valence, Tensor elements) -> "
         "(Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)")
    assert str(torch.ops.mdt.mol_key.default._schema) == "mdt::mol_key(Tensor natoms, Tensor atoms, Tensor nbonds, Tensor bonds) -> Tensor"
    assert str(torch.ops.mdt.key_flags.default._schema) == "mdt::key_flags(Tensor key, SymInt candidates, Tensor? known_key) -> Tensor"
    with FakeTensorMode():
        packed, length = torch.empty(15, 40, dtype=torch.int32), torch.empty(15, dtype=torch.int32)
        tables = (torch.empty(256, dtype=torch.uint8), torch.empty(10, dtype=torch.uint8), torch.empty(26, dtype=torch.int32))
        out = torch.ops.mdt.mol_graph(packed, length, *tables)
        assert [(tuple(t.shape), t.dtype) for t in out] == [((15,), torch.int32), ((15, 40), torch.int32), ((15,), torch.int32),
                                                            ((15, 40), torch.int32), ((15,), torch.uint8), ((15,), torch.int32)]
        key = torch.ops.mdt.mol_key(*out[:4])
        assert (tuple(key.shape), key.dtype) == ((15,), torch.int64)
        for known in (None, torch.empty(7, dtype=torch.int64)):
            flags = torch.ops.mdt.key_flags(key, 5, known)
            assert (tuple(flags.shape), flags.dtype) == ((15,), torch.uint8)
    rows, n = torch.zeros(3, 4, dtype=torch.int32), torch.zeros(3, dtype=torch.int32)      # no CPU implementation behind the ops
    v = vocabulary()
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        torch.ops.mdt.mol_graph(rows, n, *(torch.from_numpy(a) for a in (v.classes, v.max_valence, v.elements)))
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        torch.ops.mdt.mol_key(n, rows, n, rows)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        torch.ops.mdt.key_flags(torch.zeros(3, dtype=torch.int64), 3, None)


# ---------------------------------------------------------------------------------------------------------------------
# on a recording library: launch order for both identities, refusals with nothing launched
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
HEAD = ["mdt_tokens_compact", "forward_sample", "mdt_screen_score"]


def names(rec):
    return [e[0] for e in rec.log]


def test_launch_order_for_both_identities(rec):
    tok, cond, v = torch.ones(N_ * G_, L_, dtype=torch.long), torch.zeros(G_, n_), vocabulary()
    out = M.screen_tokens_diverse(Fwd(rec), tok, cond, "cpu", N_, K_, vocabulary=v, identity="graph")
    assert names(rec) == HEAD + ["mdt_smiles_check", "mdt_mol_graph", "mdt_mol_key", "mdt_key_flags", "mdt_screen_select_reject"]
    compact, _, _, check, graph, key, flags, select = rec.log
    assert graph[1:5] == check[1:5] == (compact[7], compact[8], L_, N_ * G_) and all(graph[5:14])
    assert key[1:5] == (graph[8], graph[9], graph[10], graph[11]) and key[5:7] == (L_, N_ * G_)     # the graph arrays, computed once
    assert flags[1:6] == (key[7], N_, G_, 0, 0) and flags[6] != 0
    assert len(select) == 1 + 17 and select[13] not in (0, check[8], flags[6])               # reject = the check's status | the flags
    assert out.status.shape == (N_, G_)
    # with a distance filter the diverse selection takes the same byte
    rec.log.clear()
    M.screen_tokens_diverse(Fwd(rec), tok, cond, "cpu", N_, K_, vocabulary=v, identity="graph", min_distance=3)
    assert names(rec)[3:] == ["mdt_smiles_check", "mdt_mol_graph", "mdt_mol_key", "mdt_key_flags", "mdt_screen_select_diverse_reject"]
    # with a known set: its keys are computed by the same kernels, once per (vocabulary, device)
    known = M.KnownSet(torch.ones(4, L_, dtype=torch.long), L_)
    for again in (False, True):
        rec.log.clear()
        M.screen_tokens_diverse(Fwd(rec), tok, cond, "cpu", N_, K_, vocabulary=v, identity="graph", known_tokens=known)
        middle = [] if again else ["mdt_mol_graph", "mdt_mol_key"]
        assert names(rec)[3:] == ["mdt_smiles_check", "mdt_mol_graph", "mdt_mol_key"] + middle + ["mdt_key_flags", "mdt_screen_select_reject"]
    # "string" is the call without the keyword: the same launches with the same arguments, in the same order
    for kw in (dict(), dict(vocabulary=v), dict(vocabulary=v, min_distance=2), dict(min_distance=2, known_tokens=known)):
        logs = []
        for extra in (dict(), dict(identity="string")):
            rec.log.clear()
            M.screen_tokens_diverse(Fwd(rec), tok, cond, "cpu", N_, K_, **kw, **extra)
            logs.append([(e[0], len(e), tuple(a for a in e[1:] if isinstance(a, int) and a < 4096)) for e in rec.log])
        assert logs[0] == logs[1] and not any("mol" in e[0] or "key_flags" in e[0] for e in logs[1]), kw
    # the public calls: compaction, the graph, the key
    rec.log.clear()
    key, status, position = M.mol_key(tok.to(torch.int16), v, "cpu")
    assert names(rec) == ["mdt_tokens_compact", "mdt_mol_graph", "mdt_mol_key"] and rec.log[1][3:5] == (L_, N_ * G_)
    assert key.dtype == status.dtype == position.dtype == torch.int64 and key.shape == status.shape == position.shape == (N_ * G_,)
    rec.log.clear()
    out = M.mol_graph(tok, v, "cpu")
    assert names(rec) == ["mdt_tokens_compact", "mdt_mol_graph"]
    assert [tuple(t.shape) for t in out] == [(15,), (15, L_), (15,), (15, L_), (15,), (15,)] and all(t.dtype == torch.int64 for t in out)


def test_screen_candidates_takes_the_identity(rec, monkeypatch):
    seen = {}

    class Inv:
        max_length = 32

        def sample_tokens(self, seq, device, **k):
            return torch.ones(seq.shape[0], 32, dtype=torch.long)
    monkeypatch.setattr(G, "screen_tokens", lambda *a, **k: seen.update(plain=k) or "plain")
    monkeypatch.setattr(G, "screen_tokens_diverse", lambda *a, **k: seen.update(diverse=k) or "diverse")
    cond, v = torch.zeros(2, 12), vocabulary()
    assert M.screen_candidates(Inv(), "fwd", cond, "dev", 3, 2, vocabulary=v, identity="graph", forward_timesteps=7) == "diverse"
    assert seen["diverse"] == dict(min_distance=1, min_novelty=1, vocabulary=v, identity="graph", forward_timesteps=7)
    assert M.screen_candidates(Inv(), "fwd", cond, "dev", 3, 2, identity="string", forward_timesteps=7) == "plain"
    assert seen["plain"] == dict(forward_timesteps=7)                        # as without the keyword


def test_refusals_come_before_anything_is_launched(rec):
    fwd, v = Fwd(rec), vocabulary()
    tok, cond = torch.ones(N_ * G_, L_, dtype=torch.long), torch.zeros(G_, n_)
    wide = torch.ones(N_ * G_, 65, dtype=torch.long)

    class Inv:
        max_length = 65

        def sample_tokens(self, *a, **k):
            raise AssertionError("sampled")
    for call, what in (
            (lambda: M.screen_tokens_diverse(fwd, tok, cond, "cpu", N_, K_, identity="graph"), "give a vocabulary"),
            (lambda: M.screen_tokens_diverse(fwd, wide, cond, "cpu", N_, K_, vocabulary=v, identity="graph"), "at most 64"),
            (lambda: M.screen_tokens_diverse(fwd, tok, cond, "cpu", N_, K_, vocabulary=v, identity="molecule"), "identity must be"),
            (lambda: M.screen_tokens_diverse(fwd, tok, cond, "cpu", N_, K_, identity=None), "identity must be"),
            (lambda: M.screen_candidates(Inv(), fwd, cond, "cpu", N_, K_, vocabulary=v, identity="graph"), "at most 64"),
            (lambda: M.screen_candidates(Inv(), fwd, cond, "cpu", N_, K_, identity="graph"), "give a vocabulary"),
            (lambda: M.screen_candidates(Inv(), fwd, cond, "cpu", N_, K_, identity="smiles"), "identity must be"),
            (lambda: M.mol_key(wide, v, "cpu"), "at most 64"),
            (lambda: M.mol_graph(wide, v, "cpu"), "at most 64"),
            (lambda: M.mol_key(tok[:, :0], v, "cpu"), "at least one position"),
            (lambda: M.mol_key(tok.float(), v, "cpu"), "integer"),
            (lambda: M.mol_key(tok[0], v, "cpu"), "2-D"),
            (lambda: M.mol_key(tok, S.CHARS, "cpu"), "SmilesVocabulary"),
            (lambda: M.KnownSet(wide, 65).mol_keys(v, "cpu"), "at most 64"),
            (lambda: M.KnownSet(tok, L_).mol_keys("CNO", "cpu"), "SmilesVocabulary")):
        with pytest.raises(ValueError, match=what):
            call()
    assert rec.log == []
    M.screen_tokens_diverse(fwd, wide, cond, "cpu", N_, K_, vocabulary=v)     # string identity takes wide rows as before
    assert names(rec)[-1] == "mdt_screen_select_reject"
    with pytest.raises(TypeError):                                           # screen_tokens keeps its parameter list
        M.screen_tokens(fwd, tok, cond, "cpu", N_, K_, identity="graph")
    # the ops refuse what the kernels do not take
    rec.log.clear()
    rows, n = torch.zeros(3, 65, dtype=torch.int32), torch.zeros(3, dtype=torch.int32)
    tables = [torch.from_numpy(a) for a in (v.classes, v.max_valence, v.elements)]
    with pytest.raises(RuntimeError, match="1 to 64"):
        torch.ops.mdt.mol_graph(rows, n, *tables)
    with pytest.raises(RuntimeError, match="int32 rows"):
        torch.ops.mdt.mol_graph(rows[:, :8].long(), n, *tables)
    with pytest.raises(RuntimeError, match="classes"):
        torch.ops.mdt.mol_graph(rows[:, :8], n, tables[0][:100], tables[1], tables[2])
    with pytest.raises(RuntimeError, match="1 to 64"):
        torch.ops.mdt.mol_key(n, rows, n, rows)
    with pytest.raises(RuntimeError, match="int32"):
        torch.ops.mdt.mol_key(n, rows[:, :8].long(), n, rows[:, :8])
    with pytest.raises(RuntimeError, match="one value per row"):
        torch.ops.mdt.mol_key(n[:2], rows[:, :8], n, rows[:, :8])
    with pytest.raises(RuntimeError, match="divide"):
        torch.ops.mdt.key_flags(torch.zeros(7, dtype=torch.int64), 3, None)
    with pytest.raises(RuntimeError, match="1024"):
        torch.ops.mdt.key_flags(torch.zeros(2050, dtype=torch.int64), 1025, None)
    with pytest.raises(RuntimeError, match="int64"):
        torch.ops.mdt.key_flags(torch.zeros(6, dtype=torch.int32), 3, None)
    with pytest.raises(RuntimeError, match="known_key"):
        torch.ops.mdt.key_flags(torch.zeros(6, dtype=torch.int64), 3, torch.zeros(2, dtype=torch.int32))
    assert rec.log == []


def test_known_keys_are_sorted_as_unsigned_on_int64_storage(rec, monkeypatch):
    """KnownSet.mol_keys on stand-in ops: zeros and repeats drop out, and the order is the unsigned one."""
    bits = np.array([5, 2 ** 63 + 1, 0, 2 ** 64 - 1, 5, 1, 2 ** 63, 0], dtype=np.uint64)
    known = M.KnownSet(torch.arange(1, 9).reshape(8, 1).repeat(1, 2), 4)
    assert len(known) == 8

    class Ops:
        @staticmethod
        def mol_graph(packed, length, *tables):
            return (length,) * 6

        @staticmethod
        def mol_key(*a):
            return torch.from_numpy(bits.view(np.int64).copy())
    monkeypatch.setattr(torch.ops, "mdt", Ops)
    v = vocabulary()
    keys = known.mol_keys(v, "cpu")
    assert keys.dtype == torch.int64
    assert keys.numpy().view(np.uint64).tolist() == [1, 5, 2 ** 63, 2 ** 63 + 1, 2 ** 64 - 1]
    assert known.mol_keys(v, "cpu") is keys                                  # cached per (vocabulary, device)


def test_public_surface_and_what_the_docstrings_promise():
    assert M.mol_key is G.mol_key and M.mol_graph is G.mol_graph and rt.MOL_MAX_LENGTH == G.MAX_MOL_LENGTH == 64
    import inspect
    assert "identity" not in inspect.signature(M.screen_tokens).parameters
    assert inspect.signature(M.screen_tokens_diverse).parameters["identity"].default == "string"
    for phrase in ('KEY 0 MEANS "NO MOLECULE"', "Equal graphs always give equal keys".lower(), "can collide in principle",
                   "not a canonical", "not RDKit's canonical SMILES", "[CH4] and C", "C1=CC=CC=C1 and c1ccccc1", "Stereo is ignored"):
        assert phrase in M.mol_key.__doc__ or phrase in M.mol_key.__doc__.lower(), phrase
    doc = M.screen_tokens_diverse.__doc__
    for phrase in ("in edits on the STRINGS", "((status & 8) == 0).float().mean()", "only adds bits", "the lowest c stands for all"):
        assert phrase in doc, phrase
    assert "modulo" in M.mol_graph.__doc__ and "unsigned" in M.KnownSet.mol_keys.__doc__.lower()
