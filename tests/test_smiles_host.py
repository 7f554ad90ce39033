"""No GPU: the rule set of mdt_smiles_check on its string-level reference (tests/smiles_ref.py) against the three agreed tables,
SmilesVocabulary, the C entry points' export and argument checks, the ops' schemas and shape inference, and the launch order of
the screening calls with ``vocabulary=`` on a recording library."""
import contextlib
import os
import re

import numpy as np
import pytest
import torch

import smiles_ref as S
from conftest import ROOT
import moleculediffusiontransformer_amd as M
from moleculediffusiontransformer_amd import generative as G, ops, runtime as rt


# ---------------------------------------------------------------------------------------------------------------------
# the reference and the tables
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s,status,position", S.TABLES, ids=[repr(s) for s, _, _ in S.TABLES])
def test_reference_gives_the_agreed_verdicts(s, status, position):
    assert S.check(s) == (status, position)


def test_tables_are_the_agreed_ones_and_the_mutations_reach_every_verdict():
    assert (len(S.OK_TABLE), len(S.MALFORMED_TABLE), len(S.OVERVALENT_TABLE)) == (61, 49, 14)
    assert S.check("") == (S.OK, -1)
    assert S.check("N(C)(C)(C)C", {"N": 5}) == (S.OK, -1) and S.check("C(C)(C)(C)(C)C", {"N": 5}) == (S.OVERVALENT, 0)
    rows = S.mutated_rows()
    assert len(rows) == 4096 and max(len(r) for r in rows) <= 32 and rows == S.mutated_rows()
    verdicts = [S.check(r)[0] for r in rows]
    for v in (S.OK, S.MALFORMED, S.OVERVALENT):
        assert verdicts.count(v) >= 0.05 * len(rows), (v, verdicts.count(v))


# ---------------------------------------------------------------------------------------------------------------------
# SmilesVocabulary
# ---------------------------------------------------------------------------------------------------------------------
def vocabulary(**kw):
    return M.SmilesVocabulary([None] + S.CHARS, **kw)


def test_vocabulary_round_trip_and_tables():
    v = vocabulary()
    strings = [s for s, _, _ in S.TABLES]
    ids = v.encode(strings, 32)
    assert ids.dtype == torch.int64 and ids.shape == (len(strings), 32) and v.decode(ids) == strings
    assert all(int((row != 0).sum()) == len(s) and not row[len(s):].any() for row, s in zip(ids, strings))    # zero-padded at the end
    spread = torch.zeros(len(strings), 64, dtype=torch.int64)
    spread[:, ::2] = ids                                                     # zeros anywhere: the compacted row is the string
    assert v.decode(spread) == strings and v.decode(spread.numpy().astype(np.int16)) == strings
    assert v.encode("CC", 2).tolist() == [[int(v.encode(["C"], 1)[0, 0])] * 2]     # one string stands for a list of one
    # a dict {id: char} (a keras tokenizer's index_word) gives the same tables
    d = M.SmilesVocabulary({i + 1: ch for i, ch in enumerate(S.CHARS)})
    assert np.array_equal(d.classes, v.classes) and len(d) == len(v) == len(S.CHARS)
    # the class table: letters, digits and symbols as include/mdt_hip.h numbers them; what has no character is "other"
    cls = {ch: int(v.classes[i + 1]) for i, ch in enumerate(S.CHARS)}
    assert v.classes.dtype == np.uint8 and v.classes.shape == (256,) and v.classes[0] == 0 and not v.classes[len(S.CHARS) + 1:].any()
    assert cls["l"] == 27 + 11 and cls["r"] == 27 + 17                       # halogen tails are plain lowercase letters
    assert cls["C"] == 3 and cls["B"] == 2 and cls["H"] == 8 and cls["X"] == 24 and cls["x"] == 27 + 23 and cls["c"] == 29
    assert [cls[ch] for ch in "01234"] == [53, 54, 55, 56, 57]
    assert [cls[ch] for ch in "-=#$:/\\().[]%@+*"] == list(range(63, 79))    # '@', '+', ']' mean something only inside brackets
    assert cls[" "] == 0 and G.smiles_class("é") == 0 and G.smiles_class("٣") == 0 and G.smiles_class("") == 0
    # the element table: 118 symbols, one mask per uppercase letter
    el = v.elements
    assert el.dtype == np.int32 and el.shape == (26,)
    assert sum(bin(int(w)).count("1") for w in el) == 118 == len(S.ELEMENTS)
    for sym in S.ELEMENTS:
        assert (int(el[ord(sym[0]) - 65]) >> (26 if len(sym) == 1 else ord(sym[1]) - 97)) & 1, sym
    assert not (int(el[ord("X") - 65]) >> 26) & 1 and not (int(el[ord("C") - 65]) >> (ord("x") - 97)) & 1
    # maxima and their overrides
    assert v.max_valence.tolist() == [3, 4, 3, 2, 5, 6, 1, 1, 1, 1] and v.max_valence.dtype == np.uint8
    assert vocabulary(max_valence={"N": 5, "Cl": 0}).max_valence.tolist() == [3, 4, 5, 2, 5, 6, 1, 0, 1, 1]


def test_vocabulary_refusals():
    v = vocabulary()
    for bad, what in (([None, "C", "Cl"], "exactly one character"), ({1: "C", 2: "Br"}, "exactly one character"),
                      ({0: "C"}, "outside"), ({256: "C"}, "outside"), ({-1: "C"}, "outside"), ({"1": "C"}, "integers"),
                      ({1.0: "C"}, "integers"), ({True: "C"}, "integers"), ([None] + ["C"] * 256, "outside"), ({1: 7}, "exactly one"),
                      ("CNO", "sequence"), (7, "sequence")):
        with pytest.raises(ValueError, match=what):
            M.SmilesVocabulary(bad)
    assert len(M.SmilesVocabulary([None, "C", None, "", "N"])) == 2          # None and "" are unused ids
    assert len(M.SmilesVocabulary(["ignored at index 0", "C"])) == 1
    for bad in ({"H": 1}, {"c": 3}, {"Si": 4}, {"N": 9}, {"N": -1}, {"N": 3.0}, {"N": True}):
        with pytest.raises(ValueError, match="max_valence"):
            vocabulary(max_valence=bad)
    with pytest.raises(ValueError, match="no id for"):
        v.encode(["CQ"], 8)
    with pytest.raises(ValueError, match="3 characters"):
        v.encode(["CCC"], 2)
    with pytest.raises(ValueError, match="length"):
        v.encode(["C"], 0)
    with pytest.raises(ValueError, match="no character for id 200"):
        v.decode(np.array([[1, 200]]))
    with pytest.raises(ValueError, match="integer"):
        v.decode(np.array([[1.0, 2.0]]))


# ---------------------------------------------------------------------------------------------------------------------
# header, library, binding
# ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_the_library_exports_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "mdt_hip.h")).read()
    lib = rt.load_library()
    for name in ("mdt_smiles_check", "mdt_screen_select_reject", "mdt_screen_select_diverse_reject"):
        assert re.search(r"\bint %s\s*\(" % name, hdr) and name in rt.SYMBOLS and hasattr(lib, name), name
    values = dict(re.findall(r"\b(MDT_SCREEN_[A-Z]+) = (\d+)", hdr))
    assert int(values["MDT_SCREEN_MALFORMED"]) == rt.SCREEN_MALFORMED == 32 == S.MALFORMED
    assert int(values["MDT_SCREEN_OVERVALENT"]) == rt.SCREEN_OVERVALENT == 64 == S.OVERVALENT
    assert "Not checked: aromaticity and kekulisation" in hdr
    assert len(rt.SYMBOLS["mdt_screen_select_reject"][1]) == len(rt.SYMBOLS["mdt_screen_select"][1]) + 1
    assert len(rt.SYMBOLS["mdt_screen_select_diverse_reject"][1]) == len(rt.SYMBOLS["mdt_screen_select_diverse"][1]) + 1


def test_entry_point_refuses_bad_arguments_before_any_launch():
    lib = rt.load_library()

    def check(L=32, R_=5, p=8, classes=8):
        return lib.mdt_smiles_check(p, p, L, R_, classes, p, p, p, p, 0)
    for kw, what in ((dict(L=0), b"L <= 128"), (dict(L=129), b"L <= 128"), (dict(R_=-1), b"R >= 0"), (dict(p=0), b"null"),
                     (dict(classes=0), b"null")):
        assert check(**kw) != 0, kw
        assert what in lib.mdt_last_error(), (kw, lib.mdt_last_error())
    assert check(R_=0) == 0 and check(R_=0, p=0) == 0                         # nothing to do: nothing is launched, nothing is read

    def select(reject, L=16, N=5, G_=3, K=2, p=8):
        return lib.mdt_screen_select_reject(p, p, p, p, L, N, G_, 0, 0, 0, 0, K, reject, p, p, p, 0)
    for kw, what in ((dict(N=1025), b"N <= 1024"), (dict(K=6), b"K <= N"), (dict(L=1025), b"L <= 1024"), (dict(p=0), b"null")):
        assert select(8, **kw) != 0 and what in lib.mdt_last_error(), kw
    assert lib.mdt_screen_select_diverse_reject(8, 8, 8, 8, 65, 5, 3, 0, 0, 0, 0, 2, 0, 1, 3, 8, 8, 8, 8, 0) != 0
    assert b"L <= 64" in lib.mdt_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# the ops
# ---------------------------------------------------------------------------------------------------------------------
def test_ops_schema_and_shape_inference():
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert str(torch.ops.mdt.smiles_check.default._schema) == \
        "mdt::smiles_check(Tensor packed, Tensor length, Tensor classes, Tensor max_valence, Tensor elements) -> (Tensor, Tensor)"
    assert str(torch.ops.mdt.screen_select_reject.default._schema) == \
        ("mdt::screen_select_reject(Tensor score, Tensor key, Tensor packed, Tensor length, SymInt candidates, SymInt keep, "
         "Tensor? known_key, Tensor? known_packed, Tensor? known_len, Tensor? reject) -> (Tensor, Tensor, Tensor)")
    assert str(torch.ops.mdt.screen_select_diverse_reject.default._schema) == \
        ("mdt::screen_select_diverse_reject(Tensor score, Tensor key, Tensor packed, Tensor length, SymInt candidates, SymInt keep, "
         "Tensor? known_key, Tensor? known_packed, Tensor? known_len, Tensor? known_dist, SymInt min_novelty, SymInt min_distance, "
         "Tensor? reject) -> (Tensor, Tensor, Tensor)")
    # the existing ops keep their schemas: `reject` came as new ops, not as a new argument
    assert "reject" not in str(torch.ops.mdt.screen_select.default._schema)
    assert "reject" not in str(torch.ops.mdt.screen_select_diverse.default._schema)
    with FakeTensorMode():
        packed, length = torch.empty(15, 40, dtype=torch.int32), torch.empty(15, dtype=torch.int32)
        tables = (torch.empty(256, dtype=torch.uint8), torch.empty(10, dtype=torch.uint8), torch.empty(26, dtype=torch.int32))
        status, position = torch.ops.mdt.smiles_check(packed, length, *tables)
        assert (status.shape, status.dtype, position.shape, position.dtype) == ((15,), torch.uint8, (15,), torch.int32)
        score, key = torch.empty(15), torch.empty(15, dtype=torch.int64)
        for out in (torch.ops.mdt.screen_select_reject(score, key, packed, length, 5, 2, None, None, None, status),
                    torch.ops.mdt.screen_select_diverse_reject(score, key, packed, length, 5, 2, None, None, None, None, 1, 3, status)):
            assert [(t.shape, t.dtype) for t in out] == [((15,), torch.uint8), ((3, 2), torch.int32), ((3,), torch.int32)]
    rows, n = torch.zeros(3, 4, dtype=torch.int32), torch.zeros(3, dtype=torch.int32)      # no CPU implementation behind the ops
    v = vocabulary()
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        torch.ops.mdt.smiles_check(rows, n, *(torch.from_numpy(a) for a in (v.classes, v.max_valence, v.elements)))
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        torch.ops.mdt.screen_select_reject(torch.zeros(3), torch.zeros(3, dtype=torch.int64), rows, n, 3, 1, None, None, None, None)


# ---------------------------------------------------------------------------------------------------------------------
# on a recording library: launch order with and without a vocabulary, refusals with nothing launched
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


def test_launch_order_with_a_vocabulary(rec):
    tok, cond, v = torch.ones(N_ * G_, L_, dtype=torch.long), torch.zeros(G_, n_), vocabulary()
    out = M.screen_tokens_diverse(Fwd(rec), tok, cond, "cpu", N_, K_, vocabulary=v)
    assert [e[0] for e in rec.log] == ["mdt_tokens_compact", "forward_sample", "mdt_screen_score", "mdt_smiles_check",
                                       "mdt_screen_select_reject"]
    compact, _, score, check, select = rec.log
    assert check[1:5] == (compact[7], compact[8], L_, N_ * G_) and all(check[5:10])          # packed, length, L, R; five pointers
    assert len(select) == 1 + 17 and select[13] == check[8] != 0                             # the check's status is `reject`
    assert select[1] == score[8] and select[3] == compact[7] and select[5:8] == (L_, N_, G_)
    assert out.status.shape == (N_, G_)
    # with a distance filter: the diverse selection, `reject` after (min_novelty, min_distance)
    rec.log.clear()
    M.screen_tokens_diverse(Fwd(rec), tok, cond, "cpu", N_, K_, vocabulary=v, min_distance=3)
    assert [e[0] for e in rec.log][-2:] == ["mdt_smiles_check", "mdt_screen_select_diverse_reject"]
    assert len(rec.log[-1]) == 1 + 20 and rec.log[-1][14:17] == (1, 3, rec.log[-2][8])
    # without a vocabulary: today's launches, by either name
    for call, last, arity in ((lambda: M.screen_tokens(Fwd(rec), tok, cond, "cpu", N_, K_), "mdt_screen_select", 16),
                              (lambda: M.screen_tokens_diverse(Fwd(rec), tok, cond, "cpu", N_, K_), "mdt_screen_select", 16),
                              (lambda: M.screen_tokens_diverse(Fwd(rec), tok, cond, "cpu", N_, K_, vocabulary=None, min_distance=2),
                               "mdt_screen_select_diverse", 19)):
        rec.log.clear()
        call()
        assert [e[0] for e in rec.log] == ["mdt_tokens_compact", "forward_sample", "mdt_screen_score", last]
        assert len(rec.log[-1]) == 1 + arity
    # the ops with reject=None make the existing launches
    rec.log.clear()
    packed, length, key = torch.zeros(15, 16, dtype=torch.int32), torch.zeros(15, dtype=torch.int32), torch.zeros(15, dtype=torch.int64)
    torch.ops.mdt.screen_select_reject(torch.zeros(15), key, packed, length, 5, 2, None, None, None, None)
    torch.ops.mdt.screen_select_diverse_reject(torch.zeros(15), key, packed, length, 5, 2, None, None, None, None, 1, 3, None)
    assert [(e[0], len(e)) for e in rec.log] == [("mdt_screen_select", 17), ("mdt_screen_select_diverse", 20)]
    # the public check: compaction, then one launch
    rec.log.clear()
    status, position = M.smiles_check(tok.to(torch.int16), v, "cpu")
    assert [e[0] for e in rec.log] == ["mdt_tokens_compact", "mdt_smiles_check"] and rec.log[1][3:5] == (L_, N_ * G_)
    assert status.dtype == position.dtype == torch.int64 and status.shape == position.shape == (N_ * G_,)


def test_screen_candidates_takes_the_vocabulary(rec, monkeypatch):
    seen = {}

    class Inv:
        max_length = 32

        def sample_tokens(self, seq, device, **k):
            return torch.ones(seq.shape[0], 32, dtype=torch.long)
    monkeypatch.setattr(G, "screen_tokens", lambda *a, **k: seen.update(plain=k) or "plain")
    monkeypatch.setattr(G, "screen_tokens_diverse", lambda *a, **k: seen.update(diverse=k) or "diverse")
    cond, v = torch.zeros(2, 12), vocabulary()
    assert M.screen_candidates(Inv(), "fwd", cond, "dev", 3, 2, vocabulary=v, forward_timesteps=7) == "diverse"
    assert seen["diverse"] == dict(min_distance=1, min_novelty=1, vocabulary=v, forward_timesteps=7)
    assert M.screen_candidates(Inv(), "fwd", cond, "dev", 3, 2, vocabulary=None, forward_timesteps=7) == "plain"
    assert seen["plain"] == dict(forward_timesteps=7)                        # as without the keyword


def test_refusals_come_before_anything_is_launched(rec):
    fwd, v = Fwd(rec), vocabulary()
    tok, cond = torch.ones(N_ * G_, L_, dtype=torch.long), torch.zeros(G_, n_)
    wide = torch.ones(N_ * G_, 129, dtype=torch.long)

    class Inv:
        max_length = 129

        def sample_tokens(self, *a, **k):
            raise AssertionError("sampled")
    for call, what in (
            (lambda: M.smiles_check(wide, v, "cpu"), "at most 128"),
            (lambda: M.smiles_check(tok[:, :0], v, "cpu"), "at least one position"),
            (lambda: M.smiles_check(tok.float(), v, "cpu"), "integer"),
            (lambda: M.smiles_check(tok == 1, v, "cpu"), "integer"),
            (lambda: M.smiles_check(tok[0], v, "cpu"), "2-D"),
            (lambda: M.smiles_check(tok, S.CHARS, "cpu"), "SmilesVocabulary"),
            (lambda: M.screen_tokens_diverse(fwd, wide, cond, "cpu", N_, K_, vocabulary=v), "at most 128"),
            (lambda: M.screen_tokens_diverse(fwd, tok, cond, "cpu", N_, K_, vocabulary=S.CHARS), "SmilesVocabulary"),
            (lambda: M.screen_candidates(Inv(), fwd, cond, "cpu", N_, K_, vocabulary=v), "at most 128"),
            (lambda: M.screen_candidates(Inv(), fwd, cond, "cpu", N_, K_, vocabulary="CNO"), "SmilesVocabulary")):
        with pytest.raises(ValueError, match=what):
            call()
    assert rec.log == []
    M.screen_tokens_diverse(fwd, wide, cond, "cpu", N_, K_)                   # without a vocabulary wide rows pass as before
    assert [e[0] for e in rec.log][-1] == "mdt_screen_select"
    # the ops refuse what the kernel does not take
    rows, n = torch.zeros(3, 129, dtype=torch.int32), torch.zeros(3, dtype=torch.int32)
    tables = [torch.from_numpy(a) for a in (v.classes, v.max_valence, v.elements)]
    rec.log.clear()
    with pytest.raises(RuntimeError, match="1 to 128"):
        torch.ops.mdt.smiles_check(rows, n, *tables)
    with pytest.raises(RuntimeError, match="int32 rows"):
        torch.ops.mdt.smiles_check(rows[:, :8].long(), n, *tables)
    with pytest.raises(RuntimeError, match="classes"):
        torch.ops.mdt.smiles_check(rows[:, :8], n, tables[0][:100], tables[1], tables[2])
    with pytest.raises(RuntimeError, match="max_valence"):
        torch.ops.mdt.smiles_check(rows[:, :8], n, tables[0], tables[1].int(), tables[2])
    with pytest.raises(RuntimeError, match="elements"):
        torch.ops.mdt.smiles_check(rows[:, :8], n, tables[0], tables[1], tables[2][:25])
    with pytest.raises(RuntimeError, match="reject"):
        torch.ops.mdt.screen_select_reject(torch.zeros(3), torch.zeros(3, dtype=torch.int64), rows[:, :8], n, 3, 1, None, None, None,
                                           torch.zeros(2, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="reject"):
        torch.ops.mdt.screen_select_diverse_reject(torch.zeros(3), torch.zeros(3, dtype=torch.int64), rows[:, :8], n, 3, 1, None,
                                                   None, None, None, 1, 2, torch.zeros(3, dtype=torch.int32))
    assert rec.log == []


def test_public_surface_and_what_the_docstrings_promise():
    assert M.smiles_check is G.smiles_check and M.SmilesVocabulary is G.SmilesVocabulary
    assert M.Screened._fields == ("tokens", "props", "score", "index", "count", "status")
    doc = M.smiles_check.__doc__
    for phrase in ("aromaticity and kekulisation", "two bonds between the same pair of atoms", "hydrogens", "bracket-atom valence",
                   "stereo consistency", "unverified"):
        assert phrase in doc, phrase
    assert "((status & 96) == 0).float().mean()" in M.screen_tokens_diverse.__doc__
    assert rt.SMILES_MAX_LENGTH == G.MAX_SMILES_LENGTH == 128
