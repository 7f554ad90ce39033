"""CPU: the host side of the edit distance -- the numpy reference (tests/edit_ref.py) against hand-worked cases, the three C
entry points' export, arity and argument checks, the ops' schemas and shape inference, the launch order of the diverse screening
on a recording library, and every refusal of the Python layer before anything is launched."""
import contextlib
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import moleculediffusiontransformer_amd as M
from moleculediffusiontransformer_amd import ops
from moleculediffusiontransformer_amd import runtime as rt
import edit_ref as E
import screen_ref as R


# ---------------------------------------------------------------------------------------------------------------------
# the reference against hand-worked cases
# ---------------------------------------------------------------------------------------------------------------------
def ids_of(word):
    return [ord(ch) - ord("a") + 1 for ch in word]


def test_reference_on_hand_worked_cases():
    assert E.distance(ids_of("kitten"), ids_of("sitting")) == 3
    for n in (0, 1, 7, 64):
        assert E.distance([], list(range(1, n + 1))) == n and E.distance(list(range(1, n + 1)), []) == n
    row = [1 + j % 9 for j in range(63)]
    assert E.distance(row, row) == 0
    assert E.distance([5] + row, row) == 1 and E.distance(row, [5] + row) == 1     # one insertion at the front of a 63-id row
    assert E.distance([1, 2, 3], [3, 2, 1]) == 2 and E.distance([7] * 5, [7] * 2) == 3
    # the vectorised programme == the scalar one, padded rows and every pair of lengths
    rng = np.random.default_rng(1)
    A, B = rng.integers(1, 4, (60, 7)), rng.integers(1, 4, (60, 7))
    la, lb = rng.integers(0, 8, 60), rng.integers(0, 8, 60)
    want = [E.distance(A[p, :la[p]], B[p, :lb[p]]) for p in range(60)]
    assert E.distances(A, la, B, lb).tolist() == want
    k, s = np.zeros((2, 8), np.int64), np.zeros((2, 8), np.int64)
    k[0, :6], s[0, :7] = ids_of("kitten"), ids_of("sitting")
    assert E.distances(k, [6, 0], s, [7, 0]).tolist() == [3, 0]


def test_reference_nearest_and_greedy_rules():
    Q = np.array([[1, 2, 3, 0], [4, 4, 0, 0], [0, 0, 0, 0]])
    K = np.array([[1, 2, 4, 0], [1, 2, 3, 0], [1, 2, 3, 0], [4, 0, 0, 0], [4, 4, 4, 0]])
    d, i = E.nearest(Q, [3, 2, 0], K, [3, 3, 3, 1, 3])
    assert d.tolist() == [0, 1, 1] and i.tolist() == [1, 3, 3]                # the lowest index of equal distances
    # one group: A, A' (one substitution), B (far), A'' (2 from A, 1 from A'), a NaN, an empty row, a repeat of A'
    packed = np.array([[1, 2, 3, 4, 5], [1, 2, 3, 4, 6], [7, 7, 7, 7, 7], [1, 2, 3, 9, 6], [1, 2, 3, 4, 7], [0] * 5, [1, 2, 3, 4, 6]])
    length = np.array([5, 5, 5, 5, 5, 0, 5])
    score = np.array([0.1, 0.2, 0.3, 0.4, np.nan, 0.0, 0.0], np.float32)
    st, idx, cnt = E.select_diverse(score, packed, length, 7, 1, 4, min_distance=2)
    assert st.tolist() == [0, E.CLOSE, 0, 0, R.NONFINITE, R.EMPTY, R.DUPLICATE]    # A'' is close only to the skipped A': kept
    assert idx.tolist() == [[0, 2, 3, -1]] and cnt.tolist() == [3]
    st, idx, cnt = E.select_diverse(score, packed, length, 7, 1, 4, min_distance=3)
    assert st.tolist() == [0, E.CLOSE, 0, E.CLOSE, R.NONFINITE, R.EMPTY, R.DUPLICATE] and idx.tolist() == [[0, 2, -1, -1]]
    st, idx, cnt = E.select_diverse(score, packed, length, 7, 1, 1, min_distance=2)     # CLOSE does not depend on where K stopped
    assert st.tolist() == [0, E.CLOSE, 0, 0, R.NONFINITE, R.EMPTY, R.DUPLICATE] and idx.tolist() == [[0]] and cnt.tolist() == [1]
    st, idx, cnt = E.select_diverse(score, packed, length, 7, 1, 4, known_dist=[3, 0, 1, 2, 0, 0, 0], min_novelty=2)
    assert st.tolist() == [0, R.KNOWN, R.KNOWN, 0, R.NONFINITE | R.KNOWN, R.EMPTY | R.KNOWN, R.DUPLICATE | R.KNOWN]
    same = E.select_diverse(score, packed, length, 7, 1, 4)
    for a, b in zip(same, R.select(score, packed, length, 7, 1, 4)):
        assert a.dtype == b.dtype and np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# the C entry points: exported, arity as the header, argument checks that need no device
# ---------------------------------------------------------------------------------------------------------------------
NAMES = ("mdt_edit_distance_rows", "mdt_edit_nearest", "mdt_screen_select_diverse")


def test_header_and_binding_know_the_three_functions():
    lib = rt.load_library()
    hdr = open(os.path.join(ROOT, "include", "mdt_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name)
        decl = re.search(r"\bint " + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert decl and len(decl.group(1).split(",")) == len(rt.SYMBOLS[name][1]), name
    assert [len(rt.SYMBOLS[n][1]) for n in NAMES] == [8, 11, 19]
    assert lib.mdt_abi_version() == rt.ABI_VERSION == 5                    # additions inside ABI version 5
    assert rt.SCREEN_CLOSE == E.CLOSE == 16 == int(re.search(r"MDT_SCREEN_CLOSE = (\d+)", hdr).group(1))
    assert rt.EDIT_KNOWN_CHUNK == int(re.search(r"#define MDT_EDIT_KNOWN_CHUNK (\d+)", hdr).group(1)) and rt.EDIT_KNOWN_CHUNK >= 1
    assert M.edit_distance and M.nearest_known and M.screen_tokens_diverse


def test_empty_batches_are_no_ops_and_envelope_violations_are_refused():
    lib = rt.load_library()
    assert lib.mdt_edit_distance_rows(0, 0, 0, 0, 16, 0, 0, 0) == 0
    assert lib.mdt_edit_nearest(0, 0, 16, 0, 0, 0, 5, 0, 0, 0, 0) == 0
    assert lib.mdt_screen_select_diverse(0, 0, 0, 0, 16, 5, 0, 0, 0, 0, 0, 2, 0, 1, 1, 0, 0, 0, 0) == 0

    def rows(L=16, R_=4, p=8, a=None):
        return lib.mdt_edit_distance_rows(p if a is None else a, p, p, p, L, R_, p, 0)

    def near(L=16, R_=4, M_=5, p=8, best=None):
        return lib.mdt_edit_nearest(p, p, L, R_, p, p, M_, p if best is None else best, p, p, 0)

    def select(L=16, N=5, G=3, known=(0, 0, 0), M_=0, K=2, p=8):
        return lib.mdt_screen_select_diverse(p, p, p, p, L, N, G, *known, M_, K, 0, 1, 3, p, p, p, 0)
    for call, cases in ((rows, [(dict(L=0), b"L <= 64"), (dict(L=65), b"L <= 64"), (dict(R_=-1), b"R >= 0"), (dict(p=0), b"null"),
                                (dict(a=0), b"null")]),
                        (near, [(dict(L=0), b"L <= 64"), (dict(L=65), b"L <= 64"), (dict(R_=-1), b"R >= 0"), (dict(M_=0), b"M >= 1"),
                                (dict(M_=-3), b"M >= 1"), (dict(p=0), b"null"), (dict(best=0), b"null"),
                                (dict(R_=65535 * 64 + 1), b"65535 * 64")]),
                        (select, [(dict(L=0), b"L <= 64"), (dict(L=65), b"L <= 64"), (dict(N=1025, K=2), b"N <= 1024"),
                                  (dict(N=0, K=1), b"N <= 1024"), (dict(K=0), b"K <= N"), (dict(K=6), b"K <= N"), (dict(M_=-1), b"M >= 0"),
                                  (dict(M_=3), b"M == 0"), (dict(M_=3, known=(8, 8, 0)), b"M == 0"), (dict(p=0), b"null")])):
        for kw, what in cases:
            assert call(**kw) != 0, (call.__name__, kw)
            assert what in lib.mdt_last_error(), (call.__name__, kw, lib.mdt_last_error())


# ---------------------------------------------------------------------------------------------------------------------
# the ops: schema and shape inference
# ---------------------------------------------------------------------------------------------------------------------
def test_ops_schema_and_shape_inference():
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert str(torch.ops.mdt.edit_distance.default._schema) == \
        "mdt::edit_distance(Tensor a_packed, Tensor a_len, Tensor b_packed, Tensor b_len) -> Tensor"
    assert str(torch.ops.mdt.edit_nearest.default._schema) == \
        "mdt::edit_nearest(Tensor packed, Tensor length, Tensor known_packed, Tensor known_len) -> (Tensor, Tensor)"
    assert str(torch.ops.mdt.screen_select_diverse.default._schema) == \
        ("mdt::screen_select_diverse(Tensor score, Tensor key, Tensor packed, Tensor length, SymInt candidates, SymInt keep, "
         "Tensor? known_key, Tensor? known_packed, Tensor? known_len, Tensor? known_dist, SymInt min_novelty, SymInt min_distance) "
         "-> (Tensor, Tensor, Tensor)")
    with FakeTensorMode():
        packed, length = torch.empty(15, 40, dtype=torch.int32), torch.empty(15, dtype=torch.int32)
        d = torch.ops.mdt.edit_distance(packed, length, packed, length)
        assert (d.shape, d.dtype) == ((15,), torch.int32)
        d, i = torch.ops.mdt.edit_nearest(packed, length, torch.empty(7, 40, dtype=torch.int32), torch.empty(7, dtype=torch.int32))
        assert (d.shape, d.dtype, i.shape, i.dtype) == ((15,), torch.int32, (15,), torch.int32)
        score, key = torch.empty(15), torch.empty(15, dtype=torch.int64)
        status, index, count = torch.ops.mdt.screen_select_diverse(score, key, packed, length, 5, 2, None, None, None, d, 2, 3)
        assert (status.shape, status.dtype) == ((15,), torch.uint8) and (index.shape, index.dtype) == ((3, 2), torch.int32)
        assert (count.shape, count.dtype) == ((3,), torch.int32)
    rows, n = torch.zeros(3, 4, dtype=torch.int32), torch.zeros(3, dtype=torch.int32)    # no CPU implementation behind the ops
    for call in (lambda: torch.ops.mdt.edit_distance(rows, n, rows, n), lambda: torch.ops.mdt.edit_nearest(rows, n, rows, n),
                 lambda: torch.ops.mdt.screen_select_diverse(torch.zeros(3), torch.zeros(3, dtype=torch.int64), rows, n, 3, 1, None,
                                                             None, None, None, 1, 2)):
        with pytest.raises(RuntimeError, match="no CPU implementation"):
            call()


# ---------------------------------------------------------------------------------------------------------------------
# on a recording library: the launch order of the diverse screening, and the refusals with nothing launched
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


def test_launch_order_of_the_diverse_screening(rec):
    tok, cond = torch.zeros(N_ * G_, L_, dtype=torch.long), torch.zeros(G_, n_)
    known = M.KnownSet(np.arange(1, 9).reshape(2, 4), L_)
    out = M.screen_tokens_diverse(Fwd(rec), tok, cond, "cpu", N_, K_, known_tokens=known, min_distance=3)
    assert [e[0] for e in rec.log] == ["mdt_tokens_compact", "forward_sample", "mdt_screen_score", "mdt_screen_select_diverse"]
    compact, _, score, select = rec.log
    assert select[5:8] == (L_, N_, G_) and all(select[8:11]) and select[11:13] == (2, K_)         # the key triple is passed
    assert select[13:16] == (0, 1, 3)                                                          # known_dist NULL; (novelty, distance)
    assert select[1] == score[8] and select[2] == compact[9] and select[3] == compact[7] and select[4] == compact[8]
    assert M.Screened._fields == ("tokens", "props", "score", "index", "count", "status") and out.status.shape == (N_, G_)
    # min_novelty: one nearest search over all N * G rows before the select, which gets the distances and no key triple
    rec.log.clear()
    M.screen_tokens_diverse(Fwd(rec), tok, cond, "cpu", N_, K_, known_tokens=known, min_novelty=2)
    assert [e[0] for e in rec.log] == ["mdt_tokens_compact", "forward_sample", "mdt_screen_score", "mdt_edit_nearest",
                                       "mdt_screen_select_diverse"]
    compact, _, _, near, select = rec.log
    assert near[1:3] == (compact[7], compact[8]) and near[3:5] == (L_, N_ * G_) and near[7] == 2 and all(near[5:7])
    assert select[8:12] == (0, 0, 0, 0) and select[13] == near[9] != 0 and select[14:16] == (2, 1)
    # (1, 1): today's four launches, by either name and through screen_candidates
    for call in (lambda: M.screen_tokens_diverse(Fwd(rec), tok, cond, "cpu", N_, K_, known_tokens=known, min_distance=1, min_novelty=1),
                 lambda: M.screen_tokens(Fwd(rec), tok, cond, "cpu", N_, K_, known_tokens=known)):
        rec.log.clear()
        call()
        assert [e[0] for e in rec.log] == ["mdt_tokens_compact", "forward_sample", "mdt_screen_score", "mdt_screen_select"]
        assert len(rec.log[-1]) == 1 + 16


def test_screen_candidates_takes_the_two_filters(rec, monkeypatch):
    from moleculediffusiontransformer_amd import generative as G
    seen = {}

    class Inv:
        max_length = 32

        def sample_tokens(self, seq, device, **k):
            return torch.ones(seq.shape[0], 32, dtype=torch.long)
    monkeypatch.setattr(G, "screen_tokens", lambda *a, **k: seen.update(plain=k) or "plain")
    monkeypatch.setattr(G, "screen_tokens_diverse", lambda *a, **k: seen.update(diverse=k) or "diverse")
    cond = torch.zeros(2, 12)
    assert M.screen_candidates(Inv(), "fwd", cond, "dev", 3, 2, min_distance=1, min_novelty=1, forward_timesteps=7) == "plain"
    assert seen["plain"] == dict(forward_timesteps=7)                       # as without the two keywords
    assert M.screen_candidates(Inv(), "fwd", cond, "dev", 3, 2, min_distance=3, forward_timesteps=7) == "diverse"
    assert seen["diverse"] == dict(min_distance=3, min_novelty=1, forward_timesteps=7)
    M.screen_candidates(Inv(), "fwd", cond, "dev", 3, 2, min_novelty=2, known_tokens=np.ones((4, 20), np.int64))
    assert seen["diverse"]["min_novelty"] == 2 and isinstance(seen["diverse"]["known_tokens"], M.KnownSet)


def test_refusals_come_before_anything_is_launched(rec):
    fwd = Fwd(rec)
    tok, cond = torch.ones(N_ * G_, L_, dtype=torch.long), torch.zeros(G_, n_)
    known = M.KnownSet(np.arange(1, 9).reshape(2, 4), L_)
    wide, wide_known = torch.ones(N_ * G_, 65, dtype=torch.long), M.KnownSet(np.ones((2, 4), np.int64), 65)
    big = tok.clone()
    big[7, 3] = 64
    big_known = M.KnownSet(np.array([[1, 2, 64, 3]]), L_)

    class Inv:
        max_length = 65

        def sample_tokens(self, *a, **k):
            raise AssertionError("sampled")

    class Inv32(Inv):
        max_length = 32
    for call, what in (
            (lambda: M.screen_tokens_diverse(fwd, wide, cond, "cpu", N_, K_, min_distance=2), "at most 64"),
            (lambda: M.screen_tokens_diverse(fwd, wide, cond, "cpu", N_, K_, min_novelty=2, known_tokens=wide_known), "at most 64"),
            (lambda: M.screen_candidates(Inv(), fwd, cond, "cpu", N_, K_, min_distance=2), "at most 64"),
            (lambda: M.edit_distance(wide, wide, "cpu"), "at most 64"),
            (lambda: M.nearest_known(wide, wide_known, "cpu"), "at most 64"),
            (lambda: M.screen_tokens_diverse(fwd, big, cond, "cpu", N_, K_, min_distance=2), r"ids in \[0, 64\)"),
            (lambda: M.screen_tokens_diverse(fwd, -big, cond, "cpu", N_, K_, min_distance=2), r"ids in \[0, 64\)"),
            (lambda: M.screen_tokens_diverse(fwd, tok, cond, "cpu", N_, K_, min_novelty=2, known_tokens=big_known), r"known_tokens holds ids"),
            (lambda: M.edit_distance(big, tok, "cpu"), r"a_tokens holds ids"),
            (lambda: M.edit_distance(tok, big, "cpu"), r"b_tokens holds ids"),
            (lambda: M.nearest_known(big, known, "cpu"), r"tokens holds ids"),
            (lambda: M.nearest_known(tok, big_known, "cpu"), r"known_tokens holds ids"),
            (lambda: M.nearest_known(tok, np.array([[1, 2, 64, 3]]), "cpu"), r"known_tokens holds ids"),
            (lambda: M.screen_tokens_diverse(fwd, tok, cond, "cpu", N_, K_, min_novelty=2), "non-empty known_tokens"),
            (lambda: M.screen_tokens_diverse(fwd, tok, cond, "cpu", N_, K_, min_novelty=2,
                                             known_tokens=M.KnownSet(np.zeros((0, 4), np.int64), L_)), "non-empty known_tokens"),
            (lambda: M.screen_candidates(Inv32(), fwd, cond, "cpu", N_, K_, min_novelty=2), "non-empty known_tokens"),
            (lambda: M.nearest_known(tok, np.zeros((0, 4), np.int64), "cpu"), "empty"),
            (lambda: M.nearest_known(tok, M.KnownSet(np.ones((2, 4), np.int64), 8), "cpu"), "built for rows of 8"),
            (lambda: M.edit_distance(tok, tok[:, :8], "cpu"), "same shape"),
            (lambda: M.edit_distance(tok.float(), tok, "cpu"), "integer"),
            (lambda: M.nearest_known(tok.float(), known, "cpu"), "integer")):
        with pytest.raises(ValueError, match=what):
            call()
    for name in ("min_distance", "min_novelty"):
        for bad in (0, -1, 2.0, True, "2", None):
            with pytest.raises(ValueError, match=name):
                M.screen_tokens_diverse(fwd, tok, cond, "cpu", N_, K_, known_tokens=known, **{name: bad})
            with pytest.raises(ValueError, match=name):
                M.screen_candidates(Inv(), fwd, cond, "cpu", N_, K_, known_tokens=M.KnownSet(np.ones((2, 4), np.int64), 65), **{name: bad})
    with pytest.raises(TypeError, match="unexpected"):
        M.screen_candidates(Inv(), fwd, cond, "cpu", N_, K_, min_distanse=2)
    assert rec.log == []
    # the known set's ids are looked up once and kept
    assert big_known.id_range() == (0, 64) and big_known._id_range == (0, 64) and known.id_range() == (0, 8)
    # the plain path looks at neither: ids of 64 and wide rows pass as before
    M.screen_tokens(fwd, big, cond, "cpu", N_, K_, known_tokens=big_known)
    M.screen_tokens_diverse(fwd, wide, cond, "cpu", N_, K_)
    assert [e[0] for e in rec.log].count("mdt_screen_select") == 2


def test_public_functions_compact_then_launch_once(rec):
    a = torch.tensor([[1, 0, 2, 0], [0, 0, 0, 3]], dtype=torch.int16)
    d = M.edit_distance(a, a.flip(1), "cpu")
    assert [e[0] for e in rec.log] == ["mdt_tokens_compact", "mdt_tokens_compact", "mdt_edit_distance_rows"]
    assert d.dtype == torch.int64 and d.shape == (2,) and rec.log[2][5:7] == (4, 2)
    assert rec.log[2][1:5] == (rec.log[0][7], rec.log[0][8], rec.log[1][7], rec.log[1][8])
    rec.log.clear()
    d, i = M.nearest_known(a.numpy(), np.array([[3, 0, 0, 0, 0, 0], [1, 2, 0, 0, 0, 0], [1, 2, 3, 4, 5, 0]]), "cpu")
    assert [e[0] for e in rec.log] == ["mdt_tokens_compact", "mdt_edit_nearest"]
    assert d.dtype == i.dtype == torch.int64 and d.shape == i.shape == (2,)
    assert rec.log[1][3:5] == (4, 2) and rec.log[1][7] == 2                   # the five-id known row fits no four positions
    assert "out of scope" in M.edit_distance.__doc__ and "out of scope" in M.nearest_known.__doc__
    assert "((status & 8) == 0).float().mean()" in M.screen_tokens_diverse.__doc__ and "bit 8" in M.screen_tokens_diverse.__doc__
