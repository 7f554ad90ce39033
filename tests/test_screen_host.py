"""CPU: the host side of screen_tokens() / screen_candidates() -- the numpy reference against the reference's own strings
(tests/golden/screen.npz), KnownSet, every refusal, the C entry points' argument checks, the ops' shape inference, and the launch
order of screen_tokens on a recording library."""
import contextlib
import inspect
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
import moleculediffusiontransformer_amd as M
from moleculediffusiontransformer_amd import generative as G
from moleculediffusiontransformer_amd import ops
from moleculediffusiontransformer_amd import runtime as rt
import screen_ref as R


# ---------------------------------------------------------------------------------------------------------------------
# the fixture: the reference's reverse_tokenize / is_novel on strings == equality of the compacted ids
# ---------------------------------------------------------------------------------------------------------------------
def test_fixture_covers_what_it_should():
    g = load_golden("screen.npz")
    ids, known = g["ids"], g["known_ids"]
    assert ids.shape == (40, 16) and known.shape == (10, 20) and g["novel"].dtype == np.bool_
    nz = (ids != 0).sum(axis=1)
    assert 0 in nz and 16 in nz                                            # an all-zero row and a full row
    assert any(r[0] == 0 and r.any() for r in ids)                         # leading zeros
    assert any(r[0] != 0 and (r[:np.flatnonzero(r)[-1]] == 0).any() for r in ids if r.any())      # interior zeros
    assert (known != 0).sum(axis=1).max() > 16                             # a known string longer than any row
    assert 0 < g["novel"].sum() < 40 and len(set(g["first"].tolist())) < 40


def test_reference_reproduces_the_strings_of_the_reference():
    g = load_golden("screen.npz")
    ids, alphabet = g["ids"], "".join(g["alphabet"])
    packed, length, key, _ = R.compact(ids)
    mols = [tuple(packed[b, :length[b]]) for b in range(len(ids))]
    assert ["".join(alphabet[t - 1] for t in m) for m in mols] == [str(s) for s in g["smiles"]]
    # equality classes: the first row with the same compacted ids is the first row with the same string
    assert [mols.index(m) for m in mols] == g["first"].tolist()
    assert all(key[b] == key[f] for b, f in enumerate(g["first"]))
    # novelty: one group holding every row as a candidate, against the known strings as ids
    known = [tuple(int(t) for t in row if t) for row in g["known_ids"]]
    status, index, count = R.select(np.zeros(40, np.float32), packed, length, 40, 1, 40, known)
    assert ((status & R.KNOWN) == 0).tolist() == g["novel"].tolist()
    assert ((status & R.DUPLICATE) != 0).tolist() == (g["first"] != np.arange(40)).tolist()
    assert ((status & R.EMPTY) != 0).tolist() == [s == "" for s in g["smiles"]]
    assert count[0] == (status == 0).sum() and index[0, :count[0]].tolist() == np.flatnonzero(status == 0).tolist()   # all ties


def test_reference_score_and_select_rules():
    props = np.array([[1, 2, 9], [3, 3, 9], [np.nan, 0, 9], [1, 2, 9], [np.inf, 0, 9], [0, 0, 9]], np.float32)
    target = np.array([[1, 1]], np.float32)
    s = R.score(props, target, None, 6)
    assert s[:2].tolist() == [0.5, 4.0] and np.isnan(s[2]) and np.isinf(s[4]) and s[5] == 1.0
    assert R.score(props, target, np.array([2.0, 0.0], np.float32), 6)[1] == 4.0
    packed = np.array([[5, 0], [6, 0], [7, 0], [5, 0], [8, 0], [0, 0]], np.int32)
    length = np.array([1, 1, 1, 1, 1, 0], np.int32)
    status, index, count = R.select(s, packed, length, 6, 1, 3, known=[(6,)])
    assert status.tolist() == [0, R.KNOWN, R.NONFINITE, R.DUPLICATE, R.NONFINITE, R.EMPTY]
    assert index.tolist() == [[0, -1, -1]] and count.tolist() == [1]


# ---------------------------------------------------------------------------------------------------------------------
# KnownSet and the host key
# ---------------------------------------------------------------------------------------------------------------------
def test_known_set_is_compacted_deduplicated_sorted_and_keyed():
    g = load_golden("screen.npz")
    raw = np.concatenate([g["known_ids"], g["known_ids"][[0, 3]]])         # two exact repeats
    raw[-1] = np.roll(raw[-1], 5)                                          # ... one of them with its zeros elsewhere
    ks = M.KnownSet(raw, 16)
    assert len(ks) == 9 and ks.width == 16                                 # 10 strings, the over-long one dropped
    assert ks.packed.shape == (9, 16) and ks.packed.dtype == np.int32 and ks.lengths.dtype == np.int32 and ks.key.dtype == np.uint64
    assert (np.diff(ks.key.astype(object)) >= 0).all()                     # ascending as unsigned 64-bit numbers
    want = {tuple(int(t) for t in row if t) for row in g["known_ids"] if (row != 0).sum() <= 16}
    got = [tuple(int(t) for t in ks.packed[i, :ks.lengths[i]]) for i in range(9)]
    assert set(got) == want and len(set(got)) == 9
    assert all((ks.packed[i, ks.lengths[i]:] == 0).all() for i in range(9))
    assert [int(k) for k in ks.key] == [R.row_key(m) for m in got]
    assert () in got and int(ks.key[got.index(())]) == 0                    # the empty string has key 0
    # the host key function on its own, against the reference's Python-int arithmetic; negative ids count by their 32 bits
    ids = np.array([[3, 0, -1, 7], [0, 0, 0, 0], [15, 15, 15, 15]])
    packed, length, key, _ = R.compact(ids)
    assert G.token_keys(packed, length).tolist() == key.tolist() and int(key[1]) == 0
    assert int(key[0]) == (R.mix(3) + R.mix((1 << 32) | 0xFFFFFFFF) + R.mix((2 << 32) | 7)) & R.MASK
    # tensors, narrower input than the width, an empty set; one device copy per device
    small = M.KnownSet(torch.tensor([[1, 0, 2], [0, 1, 2], [0, 0, 0]]), 5)
    assert small.packed.tolist() == sorted([[1, 2, 0, 0, 0], [0, 0, 0, 0, 0]], key=lambda r: R.row_key([t for t in r if t]))
    assert len(M.KnownSet(np.zeros((0, 4), np.int64), 8)) == 0
    k, p, n = small.on("cpu")
    assert k.dtype == torch.int64 and p.dtype == torch.int32 and n.dtype == torch.int32 and small.on("cpu")[0] is k
    for bad in (np.zeros((2, 3)), np.zeros((2, 3), bool), torch.zeros(2, 3), np.zeros(3, np.int64)):
        with pytest.raises(ValueError, match="known_tokens"):
            M.KnownSet(bad, 8)
    for bad in (0, 1025, 8.0, True):
        with pytest.raises(ValueError, match="length"):
            M.KnownSet(np.zeros((2, 3), np.int64), bad)


# ---------------------------------------------------------------------------------------------------------------------
# refusals: all of them before anything is launched (no GPU here: a launch would raise a RuntimeError instead)
# ---------------------------------------------------------------------------------------------------------------------
def models():
    inv = M.QMDiffusion(max_length=32, pred_dim=16, channels=16, context_embedding_max_length=12, text_embed_dim=64,
                        embed_dim_position=64)
    fwd = M.QMDiffusionForward(max_length=32, pred_dim=1, channels=16, context_embedding_max_length=32, text_embed_dim=64,
                               embed_dim_position=64)
    return inv, fwd


def test_argument_errors_come_before_anything_is_launched():
    inv, fwd = models()
    cond, tok = torch.zeros(3, 12), torch.zeros(15, 32, dtype=torch.long)
    for name, cases in (("candidates", [(5.0, 2), (True, 1), (0, 1), (1025, 2), ("5", 2), (None, 2)]),
                        ("keep", [(5, 2.0), (5, True), (5, 0), (5, 6), (5, None)])):
        for n, k in cases:
            with pytest.raises(ValueError, match=name):
                M.screen_tokens(fwd, tok, cond, "cuda:0", n, k)
            with pytest.raises(ValueError, match=name):
                M.screen_candidates(inv, fwd, cond, "cuda:0", n, k)
    for c in (torch.zeros(12), torch.zeros(1, 3, 12), [[0.0] * 12] * 3):
        with pytest.raises(ValueError, match="conditioning"):
            M.screen_tokens(fwd, tok, c, "cuda:0", 5, 2)
        with pytest.raises(ValueError, match="conditioning"):
            M.screen_candidates(inv, fwd, c, "cuda:0", 5, 2)
    with pytest.raises(ValueError, match="conditioning"):                   # more properties than mdt_screen_score takes
        M.screen_tokens(fwd, tok, torch.zeros(3, 65), "cuda:0", 5, 2)
    for t in (tok[:14], tok[:3], torch.zeros(16, 32, dtype=torch.long)):
        with pytest.raises(ValueError, match=r"tokens must hold candidates \* G = 15 rows"):
            M.screen_tokens(fwd, t, cond, "cuda:0", 5, 2)
    for t in (tok.float(), tok.bool(), tok.numpy().astype(np.float32)):
        with pytest.raises(ValueError, match="tokens must hold integer"):
            M.screen_tokens(fwd, t, cond, "cuda:0", 5, 2)
    with pytest.raises(ValueError, match="tokens"):
        M.screen_tokens(fwd, torch.zeros(15, 1025, dtype=torch.long), cond, "cuda:0", 5, 2)
    for w in ([1.0] * 11, [1.0] * 13, [[1.0] * 12], [1.0] * 11 + [-0.5], [1.0] * 11 + [float("nan")], [1.0] * 11 + [float("inf")],
              torch.ones(3, 12)):
        with pytest.raises(ValueError, match="weights"):
            M.screen_tokens(fwd, tok, cond, "cuda:0", 5, 2, weights=w)
        with pytest.raises(ValueError, match="weights"):
            M.screen_candidates(inv, fwd, cond, "cuda:0", 5, 2, weights=w)
    for k in (np.zeros((4, 32)), torch.zeros(4, 32), np.zeros((4, 32), bool)):
        with pytest.raises(ValueError, match="known_tokens"):
            M.screen_tokens(fwd, tok, cond, "cuda:0", 5, 2, known_tokens=k)
        with pytest.raises(ValueError, match="known_tokens"):
            M.screen_candidates(inv, fwd, cond, "cuda:0", 5, 2, known_tokens=k)
    with pytest.raises(ValueError, match="known_tokens"):                   # a KnownSet built for another row width
        M.screen_tokens(fwd, tok, cond, "cuda:0", 5, 2, known_tokens=M.KnownSet(np.zeros((1, 8), np.int64), 16))
    for cs in ([1.0, 2.0], [1.0] * 6, [[1.0] * 5], [1.0, 2.0, 3.0, 4.0, float("nan")], "x"):
        with pytest.raises(ValueError, match="cond_scale"):
            M.screen_candidates(inv, fwd, cond, "cuda:0", 5, 2, cond_scale=cs)
    with pytest.raises(TypeError, match="unexpected"):
        M.screen_candidates(inv, fwd, cond, "cuda:0", 5, 2, clamp=True)


def test_public_surface():
    p = inspect.signature(M.screen_tokens).parameters
    assert list(p) == ["model_forward", "tokens", "conditioning", "device", "candidates", "keep", "known_tokens", "weights",
                       "forward_timesteps", "X_norm_factor", "forward_noise", "sampler", "sigma_schedule"]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(p)[6:])
    assert (p["forward_timesteps"].default, p["X_norm_factor"].default, p["known_tokens"].default) == (100, 1.0, None)
    q = inspect.signature(M.screen_candidates).parameters
    assert list(q) == ["model", "model_forward", "conditioning", "device", "candidates", "keep", "cond_scale", "timesteps", "noise",
                       "screen_tokens_kwargs"]
    assert (q["cond_scale"].default, q["timesteps"].default, q["noise"].default) == (1.0, 100, None)
    assert M.Screened._fields == ("tokens", "props", "score", "index", "count", "status")
    assert "((status & 8) == 0).float().mean()" in M.screen_tokens.__doc__


def test_screen_candidates_is_one_sampling_call_then_screen_tokens(monkeypatch):
    seen = {}

    class Inv:
        max_length = 32

        def sample_tokens(self, seq, device, **k):
            seen.update(seq=seq, device=device, k=k)
            return torch.arange(seq.shape[0]).view(-1, 1).expand(-1, 32).clone()
    monkeypatch.setattr(G, "screen_tokens", lambda *a, **k: seen.update(screen=(a, k)) or "screened")
    cond = torch.arange(24.0).view(2, 12)
    out = M.screen_candidates(Inv(), "fwd", cond, "dev", 3, 2, cond_scale=[1.0, 2.0, 7.5], timesteps=9, noise="ns",
                              forward_timesteps=7, weights=[1.0] * 12)
    assert out == "screened" and torch.equal(seen["seq"], cond.repeat(3, 1)) and seen["device"] == "dev"
    assert seen["k"]["cond_scale"].tolist() == [1.0, 1.0, 2.0, 2.0, 7.5, 7.5]          # one scale per candidate block
    assert seen["k"]["timesteps"] == 9 and seen["k"]["noise"] == "ns" and seen["k"]["sampler"] is None
    a, k = seen["screen"]
    assert a[0] == "fwd" and a[1][:, 0].tolist() == list(range(6)) and a[2] is cond and a[3:] == ("dev", 3, 2)
    assert k == dict(forward_timesteps=7, weights=[1.0] * 12)
    M.screen_candidates(Inv(), "fwd", cond, "dev", 3, 2, cond_scale=2.0)
    assert seen["k"]["cond_scale"] == 2.0
    M.screen_candidates(Inv(), "fwd", cond, "dev", 3, 2, known_tokens=np.ones((4, 40), np.int64), sampler="smp")
    assert isinstance(seen["screen"][1]["known_tokens"], M.KnownSet) and seen["k"]["sampler"] == "smp"      # wrapped once


# ---------------------------------------------------------------------------------------------------------------------
# the C entry points: exported, arity as the header, argument checks that need no device
# ---------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_know_the_three_functions():
    lib = rt.load_library()
    hdr = open(os.path.join(ROOT, "include", "mdt_hip.h")).read()
    for name in ("mdt_tokens_compact", "mdt_screen_score", "mdt_screen_select"):
        assert hasattr(lib, name)
        decl = re.search(r"\bint " + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert decl and len(decl.group(1).split(",")) == len(rt.SYMBOLS[name][1]), name
    assert [len(rt.SYMBOLS[n][1]) for n in ("mdt_tokens_compact", "mdt_screen_score", "mdt_screen_select")] == [10, 9, 16]
    assert lib.mdt_abi_version() == rt.ABI_VERSION == 5                    # additions inside ABI version 5
    assert (rt.SCREEN_EMPTY, rt.SCREEN_NONFINITE, rt.SCREEN_DUPLICATE, rt.SCREEN_KNOWN) == (R.EMPTY, R.NONFINITE, R.DUPLICATE, R.KNOWN)
    assert "0x9E3779B97F4A7C15" in hdr and "0xBF58476D1CE4E5B9" in hdr and "0x94D049BB133111EB" in hdr     # the key, fixed in the header


def test_empty_batches_are_no_ops_and_envelope_violations_are_refused():
    lib = rt.load_library()
    assert lib.mdt_tokens_compact(0, 0, 16, 0, 0, 1.0, 0, 0, 0, 0) == 0
    assert lib.mdt_screen_score(0, 0, 0, 0, 0, 3, 12, 0, 0) == 0 and lib.mdt_screen_score(0, 0, 0, 0, 5, 0, 12, 0, 0) == 0
    assert lib.mdt_screen_select(0, 0, 0, 0, 16, 5, 0, 0, 0, 0, 0, 2, 0, 0, 0, 0) == 0

    def select(L=16, N=5, G=3, known=(0, 0, 0), M=0, K=2, p=8):
        return lib.mdt_screen_select(p, p, p, p, L, N, G, *known, M, K, p, p, p, 0)
    for kw, what in ((dict(N=1025, K=2), b"N <= 1024"), (dict(N=0, K=1), b"N <= 1024"), (dict(K=0), b"K <= N"), (dict(K=6), b"K <= N"),
                     (dict(L=0), b"L <= 1024"), (dict(L=1025), b"L <= 1024"), (dict(M=-1), b"M >= 0"),
                     (dict(M=3), b"M == 0"), (dict(M=3, known=(8, 8, 0)), b"M == 0"), (dict(M=3, known=(0, 8, 8)), b"M == 0"),
                     (dict(p=0), b"null")):
        assert select(**kw) != 0, kw
        assert what in lib.mdt_last_error(), (kw, lib.mdt_last_error())
    for n in (65, 0):
        assert lib.mdt_screen_score(8, 64, 8, 0, 5, 3, n, 8, 0) != 0 and b"n <= 64" in lib.mdt_last_error()
    assert lib.mdt_screen_score(8, 11, 8, 0, 5, 3, 12, 8, 0) != 0 and b"row_stride" in lib.mdt_last_error()
    assert lib.mdt_screen_score(8, 64, 0, 0, 5, 3, 12, 8, 0) != 0 and b"null" in lib.mdt_last_error()
    assert lib.mdt_screen_score(8, 64, 8, 0, 1 << 20, 1 << 12, 12, 8, 0) != 0 and b"2^31" in lib.mdt_last_error()
    assert lib.mdt_tokens_compact(8, 4, 0, 0, 0, 1.0, 16, 16, 16, 0) != 0 and b"L >= 1" in lib.mdt_last_error()
    assert lib.mdt_tokens_compact(8, 4, 16, 0, 0, 1.0, 0, 16, 16, 0) != 0 and b"null" in lib.mdt_last_error()
    assert lib.mdt_tokens_compact(8, 4, 16, 0, 0, 1.0, 8, 16, 16, 0) != 0 and b"must not be the tokens" in lib.mdt_last_error()
    assert lib.mdt_tokens_compact(8, 4, 16, 24, 0, 1.0, 16, 16, 16, 0) != 0 and b"Lf >= 1" in lib.mdt_last_error()
    for x in (0.0, float("nan"), float("inf")):
        assert lib.mdt_tokens_compact(8, 4, 16, 24, 8, x, 16, 16, 16, 0) != 0 and b"x_norm" in lib.mdt_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# the ops: schema and shape inference
# ---------------------------------------------------------------------------------------------------------------------
def test_ops_schema_and_shape_inference():
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert str(torch.ops.mdt.tokens_compact.default._schema) == \
        "mdt::tokens_compact(Tensor tokens, SymInt forward_length, float x_norm) -> (Tensor, Tensor, Tensor, Tensor)"
    assert str(torch.ops.mdt.screen_score.default._schema) == \
        "mdt::screen_score(Tensor props, Tensor target, Tensor? weights, SymInt candidates) -> Tensor"
    assert str(torch.ops.mdt.screen_select.default._schema).endswith("Tensor? known_key, Tensor? known_packed, Tensor? known_len) -> "
                                                                     "(Tensor, Tensor, Tensor)")
    with FakeTensorMode():
        tok = torch.empty(15, 40, dtype=torch.int64)
        packed, length, key, fwd = torch.ops.mdt.tokens_compact(tok, 64, 16.0)
        assert (packed.shape, packed.dtype) == ((15, 40), torch.int32) and (length.shape, length.dtype) == ((15,), torch.int32)
        assert (key.shape, key.dtype) == ((15,), torch.int64) and (fwd.shape, fwd.dtype) == ((15, 64), torch.float32)
        assert torch.ops.mdt.tokens_compact(tok[:0], 0, 1.0)[3].shape == (0, 0)
        score = torch.ops.mdt.screen_score(torch.empty(15, 1, 64), torch.empty(3, 12), None, 5)
        assert (score.shape, score.dtype) == ((15,), torch.float32)
        assert torch.ops.mdt.screen_score(torch.empty(15, 64), torch.empty(3, 12), torch.empty(12), 5).shape == (15,)
        status, index, count = torch.ops.mdt.screen_select(score, key, packed, length, 5, 2, None, None, None)
        assert (status.shape, status.dtype) == ((15,), torch.uint8) and (index.shape, index.dtype) == ((3, 2), torch.int32)
        assert (count.shape, count.dtype) == ((3,), torch.int32)
        known = (torch.empty(7, dtype=torch.int64), torch.empty(7, 40, dtype=torch.int32), torch.empty(7, dtype=torch.int32))
        assert torch.ops.mdt.screen_select(score, key, packed, length, 5, 5, *known)[1].shape == (3, 5)
    for t in (torch.zeros(3, 4, dtype=torch.long),):                       # no CPU implementation behind the ops
        with pytest.raises(RuntimeError, match="no CPU implementation"):
            torch.ops.mdt.tokens_compact(t, 0, 1.0)


# ---------------------------------------------------------------------------------------------------------------------
# screen_tokens on a recording library: compact -> forward sampling -> score -> select, once each
# ---------------------------------------------------------------------------------------------------------------------
class Recorder:
    """Stands for libmdt_hip.so: every launch is appended to ``log``."""

    def __init__(self):
        self.log = []

    def __getattr__(self, name):
        if not name.startswith("mdt_"):
            raise AttributeError(name)
        return lambda *a: self.log.append((name,) + a) or 0


def test_screen_tokens_launch_order_on_a_recording_library(monkeypatch):
    rec = Recorder()
    monkeypatch.setattr(rt, "load_library", lambda *a, **k: rec)
    monkeypatch.setattr(rt, "current_stream", lambda: 0)
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    monkeypatch.setattr(ops, "_hip", lambda *t: torch.device("cpu"))         # (the device guard: there is no device here)

    class Fwd:
        max_length = 24

        def sample(self, data, device, **k):
            rec.log.append(("forward_sample", data, k))
            return torch.zeros(data.shape[0], 1, 24)
    N, Gn, K, L, n = 5, 3, 2, 16, 12
    tok = torch.zeros(N * Gn, L, dtype=torch.long)
    known = M.KnownSet(np.arange(1, 9).reshape(2, 4), L)
    out = M.screen_tokens(Fwd(), tok, torch.zeros(Gn, n), "cpu", N, K, known_tokens=known, weights=[0.5] * n, forward_timesteps=7,
                          X_norm_factor=16.0, forward_noise="fn")
    assert [e[0] for e in rec.log] == ["mdt_tokens_compact", "forward_sample", "mdt_screen_score", "mdt_screen_select"]
    compact, fwd, score, select = rec.log
    assert compact[2:4] == (N * Gn, L) and compact[4] != 0 and compact[5:7] == (24, 16.0)       # the forward input is written
    assert fwd[1].shape == (N * Gn, 24) and fwd[1].data_ptr() == compact[4]                       # ... and sampled from in place
    assert fwd[2] == dict(cond_scale=1.0, timesteps=7, clamp=False, noise="fn", sampler=None, sigma_schedule=None)
    assert score[2] == 24 and score[4] != 0 and score[5:8] == (N, Gn, n)                          # row stride Lf; weights given
    assert select[5:8] == (L, N, Gn) and select[11:13] == (2, K) and all(select[8:11])            # M = 2 known molecules
    assert select[1] == score[8] and select[2] == compact[9] and select[3] == compact[7] and select[4] == compact[8]
    # nothing was computed here: every slot is unfilled, in the documented form
    assert out.tokens.shape == (Gn, K, L) and out.tokens.dtype == torch.int64 and not out.tokens.any()
    assert out.props.shape == (Gn, K, n) and bool(out.props.isnan().all())
    assert out.score.shape == (Gn, K) and bool(torch.isposinf(out.score).all())
    assert out.index.dtype == torch.int64 and out.index.tolist() == [[-1] * K] * Gn
    assert out.count.dtype == torch.int64 and out.count.tolist() == [0] * Gn
    assert out.status.shape == (N, Gn) and out.status.dtype == torch.uint8
    # without a known set the three pointers are NULL and M is 0
    rec.log.clear()
    M.screen_tokens(Fwd(), tok, torch.zeros(Gn, n), "cpu", N, K)
    select = rec.log[-1]
    assert select[0] == "mdt_screen_select" and select[8:12] == (0, 0, 0, 0) and rec.log[2][4] == 0
