"""CPU: the host side of refine_keep(keep_mask=) / refine_keep_tokens(keep_mask=) -- header, binding and ABI of mdt_refine_keep_enter, its
argument refusals without a device, the Python argument errors, NoiseSource(sources=), the launches of the masked run_refine on a
recording library, the shape inference of mdt::refine_keep_tokens, the wrappers, the host reference against itself, and the
fixture's own invariants."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import refine_keep_ref
from conftest import load_golden
from test_refine_host import SAMPLERS, SCHEDULE, STEP, names, rec, tiny  # noqa: F401  (rec is a fixture)
import moleculediffusiontransformer_amd as M
from moleculediffusiontransformer_amd import diffusion as D
from moleculediffusiontransformer_amd import runtime as rt

ENTRY = "mdt_refine_keep_enter"
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mdt_hip.h")


# ---------------------------------------------------------------------------------------------------------------------
# header, SYMBOLS, ABI; the refusals that need no device
# ---------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_abi_agree():
    with open(HEADER) as f:
        text = f.read()
    assert re.search(r"#define MDT_ABI_VERSION 5\b", text)
    decl = re.search(r"int " + ENTRY + r"\(([^;]*)\);", text)
    assert decl, "include/mdt_hip.h declares the entry"
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == [
        "x", "xin", "start", "step_i", "src", "draft", "keep", "keep_per_token", "n_entry", "n_src", "sigma", "c_in", "seed",
        "step_entry", "step_src", "sample0", "B", "C", "L", "Cp", "stream"]
    # the binding's ctypes, argument for argument
    ctype = lambda p: (rt._P if "*" in p else {"int32_t": rt._I, "float": rt._F, "uint64_t": rt._U64, "uint32_t": rt._U32,  # noqa: E731
                                               "int64_t": rt._L}[p.split()[0]])
    res, args = rt.SYMBOLS[ENTRY]
    assert res is rt._I and args == [ctype(p) for p in params]
    comment = text[:decl.start()].rsplit("/*", 1)[1]
    assert "An addition inside ABI version 5" in comment
    lib = rt.load_library()
    assert hasattr(lib, ENTRY) and lib.mdt_abi_version() == rt.ABI_VERSION == 5


def test_entry_refusals_without_a_device():
    """Every call below with B > 0 is refused before anything is launched (the pointers are not real)."""
    lib = rt.load_library()

    def call(x=8, xin=8, start=8, src=8, draft=0, keep=8, B=1, C=16, L=32, Cp=16):
        return lib.mdt_refine_keep_enter(x, xin, start, 3, src, draft, keep, 1, 0, 0, 1.0, 1.0, 7, 0, 11, 0, B, C, L, Cp, 0)
    assert call(x=0, xin=0, start=0, src=0, keep=0, B=0) == 0                   # B <= 0: nothing to do
    assert call(src=0) != 0 and b"dense" in lib.mdt_last_error()                # no source
    assert call(draft=8) != 0 and b"dense" in lib.mdt_last_error()              # both sources
    for null in ("x", "xin", "start", "keep"):
        assert call(**{null: 0}) != 0 and b"null" in lib.mdt_last_error(), null
    assert b"mdt_refine_keep_enter" in lib.mdt_last_error()
    assert call(L=30) != 0 and b"L % 4" in lib.mdt_last_error()
    assert call(C=22) != 0                                                      # Cp < C
    assert call(Cp=24) != 0                                                     # Cp % 16
    assert call(L=4096) != 0 and b"LDS" in lib.mdt_last_error()                 # the (L, Cp) tile does not fit
    assert call(src=0, draft=8, keep=0) != 0 and b"null" in lib.mdt_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# Python surface
# ---------------------------------------------------------------------------------------------------------------------
def test_surface_has_the_keyword_with_default_none():
    """refine() / refine_tokens() / refine_tokens_sharded keep their pinned signatures (test_refine_host.test_class_surface); the
    mask is an argument of their refine_keep siblings, which take everything else as they do."""
    from moleculediffusiontransformer_amd.distributed import refine_keep_tokens_sharded, refine_tokens_sharded
    for fn in (M.QMDiffusion.refine_keep, M.QMDiffusion.refine_keep_tokens, M.refine_and_validate, refine_keep_tokens_sharded):
        p = inspect.signature(fn).parameters["keep_mask"]
        assert p.default is None and p.kind in (inspect.Parameter.KEYWORD_ONLY, inspect.Parameter.POSITIONAL_OR_KEYWORD), fn
    for sibling, plain in ((M.QMDiffusion.refine_keep, M.QMDiffusion.refine),
                           (M.QMDiffusion.refine_keep_tokens, M.QMDiffusion.refine_tokens),
                           (refine_keep_tokens_sharded, refine_tokens_sharded)):
        s, q = inspect.signature(sibling).parameters, inspect.signature(plain).parameters
        assert list(s) == list(q) + ["keep_mask"]
        assert all(s[k].kind is q[k].kind and s[k].default == q[k].default for k in q), sibling
    assert inspect.signature(M.QMDiffusion.refine_keep).parameters["keep_mask"].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(M.QMDiffusion.refine_keep_tokens).parameters["keep_mask"].kind is inspect.Parameter.KEYWORD_ONLY
    assert M.QMDiffusionForward.refine_keep_tokens is M.QMDiffusion.refine_keep_tokens
    r = inspect.signature(D.run_refine).parameters
    assert r["keep"].default is None and r["keep"].kind is inspect.Parameter.KEYWORD_ONLY
    assert r["keep_per_token"].kind is inspect.Parameter.KEYWORD_ONLY
    n = inspect.signature(D.NoiseSource.__init__).parameters
    assert list(n) == ["self", "init", "steps", "seed", "sample0", "sources"] and n["sources"].default is None


def test_argument_errors_come_before_anything_is_launched():
    m = tiny()
    seq, draft, src = torch.zeros(3, 12), torch.zeros(3, 32, dtype=torch.long), torch.zeros(3, 16, 32)
    tok_mask, full_mask = torch.zeros(3, 32, dtype=torch.bool), torch.zeros(3, 16, 32, dtype=torch.bool)
    # (no GPU here: anything that got as far as the embedding would raise a RuntimeError instead)
    for bad in (tok_mask.long(), tok_mask.float(), tok_mask.to(torch.uint8), tok_mask[:2], tok_mask[:, :31], full_mask[:, :15],
                full_mask, tok_mask[0]):
        with pytest.raises(ValueError, match="keep_mask"):
            m.refine_keep_tokens(seq, "cuda:0", draft, 3, timesteps=8, keep_mask=bad)
    for bad in (full_mask.long(), full_mask.float(), full_mask[:2], full_mask[:, :15], full_mask[:, :, :31], tok_mask[:, :31], tok_mask[0]):
        with pytest.raises(ValueError, match="keep_mask"):
            m.refine_keep(seq, "cuda:0", src, 3, timesteps=8, keep_mask=bad)
    # the other arguments are refused as without a mask
    with pytest.raises(ValueError, match="start_step"):
        m.refine_keep_tokens(seq, "cuda:0", draft, 7, timesteps=8, keep_mask=tok_mask)
    with pytest.raises(ValueError, match="source"):
        m.refine_keep(seq, "cuda:0", src[:, :15], 3, timesteps=8, keep_mask=full_mask)

    class Own(D.ADPM2Sampler):
        def step(self, x, fn, sigma, sigma_next, **k):
            return x
    for smp in (D.Sampler(), Own()):
        with pytest.raises(TypeError, match="needs the fused loop"):
            m.refine_keep_tokens(seq, "cuda:0", draft, 3, timesteps=8, sampler=smp, keep_mask=tok_mask)
        with pytest.raises(TypeError, match="needs the fused loop"):
            m.refine_keep(seq, "cuda:0", src, 3, timesteps=8, sampler=smp, keep_mask=full_mask)
    # an empty batch: empty results, on any device
    tok, x = m.refine_keep_tokens(seq[:0], "cpu", draft[:0], 3, timesteps=8, return_sample=True, keep_mask=tok_mask[:0])
    assert tok.shape == (0, 32) and x.shape == (0, 16, 32)
    assert m.refine_keep(seq[:0], "cpu", src[:0], 3, timesteps=8, keep_mask=full_mask[:0]).shape == (0, 16, 32)


def test_run_refine_mask_refusals(rec):  # noqa: F811
    emb, draft, src = torch.zeros(3, 12, 128), torch.zeros(3, 32, dtype=torch.long), torch.zeros(3, 16, 32)
    tok_mask, full_mask = torch.zeros(3, 32, dtype=torch.bool), torch.zeros(3, 16, 32, dtype=torch.bool)
    args = (rec, emb, 16, 8, D.NoiseSource(seed=1), SCHEDULE, D.ADPM2Sampler(rho=1), 0.1, 3)
    for keep, per_token in ((tok_mask, False), (full_mask, True), (tok_mask.to(torch.uint8), True), (full_mask.float(), False),
                            (tok_mask[:2], True)):
        with pytest.raises(ValueError, match="keep"):
            D.run_refine(*args, draft=draft, keep=keep, keep_per_token=per_token)
    # explicit (init, steps) noise and a mask: sources is required -- and is not where there is no mask
    zeros = torch.zeros(3, 16, 32)
    explicit = D.NoiseSource(init=zeros, steps=lambda i: zeros)
    assert explicit.sources is None and D.NoiseSource(seed=3).sources is None
    with pytest.raises(ValueError, match="sources"):
        D.run_refine(rec, emb, 16, 8, explicit, SCHEDULE, D.ADPM2Sampler(rho=1), 0.1, 3, source=src, keep=full_mask)
    assert rec.log == []                                              # all of it before anything is launched
    D.run_refine(rec, emb, 16, 8, explicit, SCHEDULE, D.ADPM2Sampler(rho=1), 0.1, 3, source=src)
    assert "mdt_refine_enter" in names(rec.log) and ENTRY not in names(rec.log)


# ---------------------------------------------------------------------------------------------------------------------
# the masked loop on the recording library
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(SAMPLERS))
@pytest.mark.parametrize("start", [2, [3, 1, 3, 5]])
@pytest.mark.parametrize("explicit", [True, False])
def test_masked_run_refine_launches(rec, kind, start, explicit):  # noqa: F811
    """mdt_refine_keep_enter once in front of every step from min(start) (for Karras in front of mdt_karras_hat), with the draws
    0 (entry), T + i (source) and i + 1 (step); no mdt_refine_enter; the last update kernel does not decode; mdt_inpaint_finish once,
    after the last step; no draw and no source draw is asked below min(start)."""
    T, B = 8, 4
    sampler = SAMPLERS[kind]()
    asked, asked_src = [], []
    init = torch.zeros(B, 16, 32)
    src_draws = {}

    def sources(i):
        asked_src.append(i)
        return src_draws.setdefault(i, torch.zeros(B, 16, 32))
    if explicit:
        ns = D.NoiseSource(init=init, steps=lambda i: asked.append(i) or torch.zeros(B, 16, 32), sources=sources)
    else:
        ns = D.NoiseSource(seed=77, sample0=5, sources=sources)       # (sources is not consulted in seed mode)
    draft = torch.zeros(B, 32, dtype=torch.long)
    keep = torch.zeros(B, 32, dtype=torch.bool)
    keep[:, ::3] = True
    tok = torch.zeros(B, 32, dtype=torch.int32)
    x = D.run_refine(rec, torch.zeros(B, 12, 128), 16, T, ns, SCHEDULE, sampler, 0.1, start, draft=draft, tokens=tok, keep=keep,
                     keep_per_token=True)
    assert x.shape == (B, 16, 32)
    sigmas, steps = D.FUSED_SAMPLERS[kind].plan(T, SCHEDULE, sampler, 0.1)
    assert torch.equal(rec.times, torch.tensor(D.plan_time_rows(steps), dtype=torch.float32))      # the full call's time table
    starts = [start] * B if isinstance(start, int) else start
    kmin = min(starts)
    per_step, drawer, at = STEP[kind]
    assert names(rec.log) == ([ENTRY] + per_step) * (T - 1 - kmin) + ["mdt_inpaint_finish"]
    assert asked == (list(range(kmin, T - 1)) if explicit else [])
    assert asked_src == (list(range(kmin, T - 1)) if explicit else [])
    assert [e[at + 1] for e in rec.log if e[0] == drawer] == list(range(kmin + 1, T))               # step i takes draw i + 1
    evals = 1 if kind == "aeuler" else 2
    assert [e[1] for e in rec.log if e[0] == "time"] == list(range(evals * kmin, evals * (T - 1)))
    enters = [e for e in rec.log if e[0] == ENTRY]
    assert [e[4] for e in enters] == list(range(kmin, T - 1))
    state = {e[1] for e in rec.log if e[0] == per_step[0]}            # the buffers the steps read as their state
    for e in enters:
        i = e[4]
        s = steps[i]
        assert e[1] in state and e[2] == rec.xin.data_ptr() and e[3] != 0
        assert e[5] == 0 and e[6] != 0 and e[7] != 0 and e[8] == 1    # token form, a per-token mask
        assert e[9] == (init.data_ptr() if explicit else 0)           # the entry noise
        assert e[10] == (src_draws[i].data_ptr() if explicit else 0)  # the source draw of step i
        assert e[11] == float(sigmas[i]) and e[12] == (s.w_hat if kind == "karras" else s.w).c_in
        assert e[13] == (0 if explicit else 77) and e[14] == 0 and e[15] == T + i and e[16] == (0 if explicit else 5)
        assert tuple(e[17:21]) == (B, 16, 32, 16)
    # the decode is mdt_inpaint_finish's, not the last update kernel's
    for e in rec.log:
        if e[0] in per_step:
            assert tok.data_ptr() not in e[1:]
    fin = rec.log[-1]
    assert fin[0] == "mdt_inpaint_finish" and fin[2] == 0 and fin[3] == enters[0][6] and fin[4] == enters[0][7] and fin[5] == 1
    assert fin[6] == tok.data_ptr() and tuple(fin[7:10]) == (B, 16, 32)


def test_masked_run_refine_clamps_after_the_merge_and_traces(rec):  # noqa: F811
    B, T = 3, 6
    src, keep = torch.zeros(B, 16, 32), torch.zeros(B, 16, 32, dtype=torch.bool)
    tok, trace = torch.zeros(B, 32, dtype=torch.int32), {"want": (3, T - 1)}
    D.run_refine(rec, torch.zeros(B, 12, 128), 16, T, D.NoiseSource(seed=1), SCHEDULE, D.AEulerSampler(), 0.1, 2, source=src,
                 tokens=tok, keep=keep, clamp=True, trace=trace, embedding_scale=[1.0, 2.0, 3.0], dynamic_threshold=0.9)
    tail = names(rec.log)[-3:]
    assert tail == ["mdt_inpaint_finish", "mdt_clamp", "mdt_argmax_tokens"]           # merge, clamp, then the decode of the clamped
    fin = [e for e in rec.log if e[0] == "mdt_inpaint_finish"][0]
    assert fin[2] != 0 and fin[3] == 0 and fin[5] == 0                # dense source, a full-shape mask
    assert sorted(k for k in trace if k != "want") == [3, T - 1]
    assert names(rec.log).count("mdt_cfg_mix_rows") == T - 1 - 2 and names(rec.log).count("mdt_dyn_scale") == T - 1 - 2
    assert names(rec.log).count(ENTRY) == T - 1 - 2 and "mdt_refine_enter" not in names(rec.log)


# ---------------------------------------------------------------------------------------------------------------------
# the op, the wrappers
# ---------------------------------------------------------------------------------------------------------------------
def test_refine_keep_tokens_op_schema_and_shape_inference():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from moleculediffusiontransformer_amd import ops  # noqa: F401  (registers torch.ops.mdt.*)
    schema = str(torch.ops.mdt.refine_keep_tokens.default._schema)
    assert schema.startswith("mdt::refine_keep_tokens(Tensor embedding, Tensor draft, Tensor start, Tensor keep, Tensor? init_noise, "
                             "Tensor sigmas, ")
    assert "sampler_kind" in schema and "float[] sampler_params" in schema and schema.endswith("-> (Tensor, Tensor)")
    # mdt::refine_tokens keeps its schema
    assert str(torch.ops.mdt.refine_tokens.default._schema).startswith(
        "mdt::refine_tokens(Tensor embedding, Tensor draft, Tensor start, Tensor? init_noise, Tensor sigmas, ")
    with FakeTensorMode():
        emb, sig = torch.empty(5, 12, 128), torch.empty(9)
        draft, start = torch.empty(5, 32, dtype=torch.int64), torch.empty(5, dtype=torch.int32)
        keep = torch.empty(5, 32, dtype=torch.bool)
        x, tok = torch.ops.mdt.refine_keep_tokens(emb, draft, start, keep, None, sig, 1, 22, 0, [1.0], 0.1, 2.0, 7, 0, 0.0)
        assert x.shape == (5, 22, 32) and x.dtype == torch.float32
        assert tok.shape == (5, 32) and tok.dtype == torch.int32
        x, tok = torch.ops.mdt.refine_keep_tokens(emb[:0], draft[:0], start[:0], keep[:0], torch.empty(0, 16, 32), sig, 1, 16, 1, [],
                                                  0.1, 1.0, 7, 3)
        assert x.shape == (0, 16, 32) and tok.shape == (0, 32)


def test_strength_sweep_repeats_the_mask_per_strength():
    seen = {}

    class Model:
        def refine_tokens(self, seq, device, draft, **k):
            seen.update(k=k, masked=False)
            return torch.zeros(seq.shape[0], 32, dtype=torch.long)

        def refine_keep_tokens(self, seq, device, draft, **k):
            seen.update(k=k, masked=True)
            return torch.zeros(seq.shape[0], 32, dtype=torch.long)
    seq, draft = torch.arange(24.0).view(2, 12), torch.arange(64).view(2, 32) % 16
    keep = torch.arange(64).view(2, 32) % 3 == 0
    tok = M.strength_sweep(Model(), seq, draft, [0.25, 0.5, 1.0], "dev", timesteps=64, keep_mask=keep)
    assert tok.shape == (3, 2, 32) and seen["masked"] and torch.equal(seen["k"]["keep_mask"], keep.repeat(3, 1))
    assert seen["k"]["start_step"].tolist() == [47, 47, 31, 31, 0, 0]
    M.strength_sweep(Model(), seq, draft, [0.5], "dev", timesteps=64)
    assert "keep_mask" not in seen["k"] and not seen["masked"]
    M.strength_sweep(Model(), seq, draft, [0.5], "dev", timesteps=64, keep_mask=None)
    assert "keep_mask" not in seen["k"] and not seen["masked"]


def test_refine_and_validate_hands_the_mask_on(monkeypatch):
    from moleculediffusiontransformer_amd import generative as G
    seen = {}

    class Inv:
        def refine_keep_tokens(self, *a, **k):
            seen["k"] = k
            return torch.full((2, 32), 3)
    monkeypatch.setattr(G, "predict_properties_from_tokens", lambda mf, tok, dev, **k: "props")
    cond, draft, keep = torch.zeros(2, 12), torch.ones(2, 32, dtype=torch.long), torch.ones(2, 32, dtype=torch.bool)
    tok, props = M.refine_and_validate(Inv(), "fwd", cond, draft, "cpu", 3, timesteps=9, keep_mask=keep)
    assert seen["k"]["keep_mask"] is keep and props == "props"


def test_sharded_wrapper_slices_the_mask_with_the_draft(monkeypatch):
    from moleculediffusiontransformer_amd import distributed as dd
    total = 7
    seq = torch.arange(total * 4, dtype=torch.float32).view(total, 4)
    draft = (torch.arange(total * 8).view(total, 8) * 7) % 16
    keep = (torch.arange(total * 8).view(total, 8) % 3) == 0
    start = [(3 * b) % 6 for b in range(total)]
    # rank 1 of 2, without a process group: the collective stands aside
    monkeypatch.setattr(dd.dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dd.dist, "get_world_size", lambda group=None: 2)
    monkeypatch.setattr(dd.dist, "get_rank", lambda group=None: 1)
    monkeypatch.setattr(dd, "all_gather_tokens", lambda local, n, vocab, group: local)
    lo, hi = dd.shard_bounds(total, 2, 1)
    seen = {}

    def local(s, d, st, first, **more):
        seen.update(s=s, d=d, st=st, first=first, more=more)
        return d
    dd.refine_keep_tokens_sharded(local, seq, draft, start, vocab=16, keep_mask=keep)
    assert 0 < lo < hi == total and seen["first"] == lo
    assert torch.equal(seen["d"], draft[lo:hi]) and list(seen["st"]) == start[lo:hi]
    assert list(seen["more"]) == ["keep_mask"] and torch.equal(seen["more"]["keep_mask"], keep[lo:hi])
    dd.refine_tokens_sharded(local, seq, draft, start, vocab=16)
    assert seen["more"] == {}                                          # without a mask the callback is called as before
    with pytest.raises(ValueError, match="keep_mask"):
        dd.refine_keep_tokens_sharded(local, seq, draft, start, vocab=16, keep_mask=keep[:-1])


# ---------------------------------------------------------------------------------------------------------------------
# the host reference: known answers
# ---------------------------------------------------------------------------------------------------------------------
def test_host_reference_known_answers():
    B, C, L, Cp = 4, 3, 8, 16
    rng = np.random.default_rng(5)
    x, xin = rng.standard_normal((B, C, L)).astype(np.float32), np.full((B, L, Cp), 9.0, np.float32)
    src = rng.standard_normal((B, C, L)).astype(np.float32)
    ne, ns = rng.standard_normal((B, C, L)).astype(np.float32), rng.standard_normal((B, C, L)).astype(np.float32)
    keep = np.zeros((B, L), bool)
    keep[:, 1::3] = True
    start, i, sigma, c_in = [2, 3, 4, 3], 3, np.float32(1.7), np.float32(0.3)
    xo, xino, runs = refine_keep_ref.keep_enter(x, xin, start, i, sigma, c_in, keep, src=src, n_entry=ne, n_src=ns)
    assert runs.tolist() == [True, True, False, True] and xo.dtype == np.float32
    assert np.array_equal(xo[2], x[2]) and np.array_equal(xino[2], xin[2])                         # not started: untouched
    k3 = np.repeat(keep[:, None, :], C, axis=1)
    merged = src + (sigma * ns).astype(np.float32)
    entered = src + (sigma * ne).astype(np.float32)
    assert np.array_equal(xo[runs][k3[runs]], merged[runs][k3[runs]])
    assert np.array_equal(xo[0][~k3[0]], x[0][~k3[0]])                                             # started: free positions stay
    assert np.array_equal(xo[1][~k3[1]], entered[1][~k3[1]])                                       # entering: noised source
    assert np.array_equal(xino[0][:, :C], (c_in * xo[0]).T) and not xino[0][:, C:].any()
    # an all-False mask is refine_ref.refine_enter on the entering rows, and leaves a started row's state alone
    import refine_ref
    xo2, xino2, _ = refine_keep_ref.keep_enter(x, xin, start, i, sigma, c_in, np.zeros((B, C, L), bool), src=src, n_entry=ne, n_src=ns)
    wx, wxin, entering = refine_ref.refine_enter(x, xin, start, i, sigma, c_in, src=src, noise=ne)
    assert np.array_equal(xo2[entering], wx[entering]) and np.array_equal(xino2[entering], wxin[entering])
    assert np.array_equal(xo2[0], x[0])
    # the last merge and the decode
    draft = rng.integers(0, C, (B, L))
    out, tok = refine_keep_ref.finish(x, keep, draft=draft)
    assert np.array_equal(tok[keep], draft[keep]) and np.array_equal(tok[~keep], x.argmax(axis=1)[~keep])
    assert np.array_equal(out[k3], refine_ref.one_hot(draft, C)[k3]) and np.array_equal(out[~k3], x[~k3])


# ---------------------------------------------------------------------------------------------------------------------
# the fixture
# ---------------------------------------------------------------------------------------------------------------------
CASES = {"a": ("tiny", "adpm2", 1.0, [4, 4, 4], "mix"), "b": ("tiny", "adpm2", 2.0, [1, 1, 1], "edge"),
         "c": ("pd22", "adpm2", 2.0, [3, 3, 3], "mix"), "d": ("pd22", "aeuler", 2.0, [0, 0, 0], "edge"),
         "e": ("tiny", "aeuler", 2.0, [2, 2, 2], "mix"), "f": ("pd22", "aeuler", 1.0, [1, 1, 1], "edge"),
         "g": ("pd22", "adpm2", 1.0, [0, 0, 0], "edge"), "rows": ("tiny", "adpm2", 2.0, [1, 3, 5], "mix")}


def test_fixture_invariants():
    g = load_golden("refine_keep.npz")
    assert [str(c) for c in g["cases"]] == list(CASES)
    changed = 0
    for (name, (model, sampler, cs, start, mask)), gm, gs, gk, gt in zip(CASES.items(), g["models"], g["samplers"], g["masks"], g["tags"]):
        assert (str(gm), str(gs), str(gk), str(gt)) == (model, sampler, mask, f"rk_{model}")
        C = {"tiny": 16, "pd22": 22}[model]
        assert g[f"{name}_seq"].shape == (3, 12) and g[f"{name}_draft"].shape == (3, 32) and g[f"{name}_out"].shape == (3, C, 32)
        assert g[f"{name}_keep"].shape == (3, 32) and g[f"{name}_keep"].dtype == np.bool_
        assert g[f"{name}_out"].dtype == np.float32 and g[f"{name}_tokens"].shape == (3, 32)
        assert g[f"{name}_start"].tolist() == start and int(g[f"{name}_timesteps"]) == 8 and float(g[f"{name}_cond_scale"]) == cs
        keep, draft = torch.from_numpy(g[f"{name}_keep"]), torch.from_numpy(g[f"{name}_draft"])
        out, tokens = torch.from_numpy(g[f"{name}_out"]), torch.from_numpy(g[f"{name}_tokens"])
        # the masks: 'mix' has kept and free positions in every row and changes inside a group of four; 'edge' has a fully kept
        # and a fully free row
        per_row = keep.sum(dim=1).tolist()
        if mask == "mix":
            assert all(0 < n < 32 for n in per_row)
            quads = keep.view(3, 8, 4).sum(dim=2)
            assert bool(((quads > 0) & (quads < 4)).any())
        else:
            assert 32 in per_row and 0 in per_row
        # (b) kept positions equal the source exactly, and decode to the draft
        full = keep.unsqueeze(1).expand(3, C, 32)
        assert torch.equal(out[full], M.one_hot_draft(draft, C)[full]) and torch.equal(tokens[keep], draft[keep])
        # (c) tokens are the argmax of the sample, and EVERY position's top-two margin is above twice the 1e-4 sample tolerance
        assert torch.equal(out.argmax(dim=1), tokens)
        top2 = torch.topk(out, 2, dim=1).values
        margin = (top2[:, 0] - top2[:, 1]).flatten(1).min(dim=1).values
        assert torch.equal(margin, torch.from_numpy(g[f"{name}_margin"])) and float(margin.min()) > 2e-4
        changed += int((tokens != draft)[~keep].sum())
    # (d) the fixture tests more than the identity
    assert changed == int(g["free_tokens_changed"]) > 0
    # the per-sample case is stitched from scalar runs: the same inputs as case a's model
    assert np.array_equal(g["rows_draft"], g["a_draft"]) and np.array_equal(g["rows_keep"], g["a_keep"])
