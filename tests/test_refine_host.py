"""CPU: the host side of refine() / refine_tokens() -- refine_start and the start-step normalisation, every refusal, the launches
of run_refine and run_sampler on a recording library (plan, time rows, draws, the entry launches), the shape inference of
mdt::refine_tokens, the chain and sweep wrappers, the sharded wrapper under gloo, and the fixture's own identities."""
import contextlib
import inspect
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import load_golden
import moleculediffusiontransformer_amd as M
from moleculediffusiontransformer_amd import diffusion as D
from moleculediffusiontransformer_amd import runtime as rt

SCHEDULE = D.KarrasSchedule(0.001, 9.0, 3.0)


def tiny():
    return M.QMDiffusion(max_length=32, pred_dim=16, channels=16, context_embedding_max_length=12, text_embed_dim=64,
                         embed_dim_position=64)


# ---------------------------------------------------------------------------------------------------------------------
# refine_start / start_rows
# ---------------------------------------------------------------------------------------------------------------------
def test_refine_start_values():
    # steps_run = min(T - 1, max(1, ceil(strength * (T - 1)))), start = T - 1 - steps_run
    want = {(2, 1e-9): 0, (2, 0.5): 0, (2, 1.0): 0,
            (8, 1e-9): 6, (8, 0.5): 3, (8, 1.0): 0,
            (64, 1e-9): 62, (64, 0.5): 31, (64, 1.0): 0}
    for (T, s), start in want.items():
        assert D.refine_start(T, s) == start == M.refine_start(T, s), (T, s)
        assert 0 <= start <= T - 2
    assert D.refine_start(64, [0.25, 0.5, 1.0]) == [47, 31, 0]
    assert D.refine_start(8, torch.tensor([1e-9, 0.5])) == [6, 3] and D.refine_start(8, np.array([1.0])) == [0]
    assert D.refine_start(8, torch.tensor(0.5)) == 3
    for bad in (0.0, -0.1, 1.0001, float("nan"), True, "0.5", [0.5, 0.0], [[0.5]], None):
        with pytest.raises(ValueError, match="strength"):
            D.refine_start(8, bad)
    for T in (1, 0, 8.0, True):
        with pytest.raises(ValueError, match="timesteps"):
            D.refine_start(T, 0.5)


def test_start_rows_normalisation_and_refusals():
    assert D.start_rows(3, 4, 8) == 3 and isinstance(D.start_rows(3, 4, 8), int)
    assert D.start_rows(torch.tensor(6), 4, 8) == 6 and D.start_rows(np.int64(0), 4, 8) == 0
    for same in ([2, 2, 2, 2], (2, 2, 2, 2), np.array([2, 2, 2, 2]), torch.tensor([2, 2, 2, 2], dtype=torch.int32)):
        got = D.start_rows(same, 4, 8)                       # all equal: the scalar call
        assert got == 2 and isinstance(got, int)
    rows = D.start_rows([0, 6, 3, 3], 4, 8)
    assert isinstance(rows, torch.Tensor) and rows.dtype == torch.int32 and rows.tolist() == [0, 6, 3, 3]
    assert rows.device.type == "cpu" and rows.is_contiguous()
    assert D.start_rows([], 0, 8) == 0                       # an empty batch
    bad = [2.0, True, None, 1 + 0j, "3", -1, 7, [1, 2, 3], [1, 2, 3, 4, 5], [1, 2, 3, 7], [0, -1, 2, 3], [1.0, 2.0, 3.0, 4.0],
           [True, False, True, True], [[1, 2, 3, 4]], torch.tensor([1.5, 2, 3, 4]), np.array([1, 2, 3, 4], dtype=np.float32),
           torch.tensor(2.0)]
    for v in bad:
        with pytest.raises(ValueError, match="start_step"):
            D.start_rows(v, 4, 8)
    with pytest.raises(ValueError, match="my_name"):
        D.start_rows(9, 4, 8, "my_name")
    with pytest.raises(ValueError, match="timesteps"):
        D.start_rows(0, 4, 1)


def test_class_surface():
    p = inspect.signature(M.QMDiffusion.refine).parameters
    assert list(p) == ["self", "sequences", "device", "source", "start_step", "cond_scale", "timesteps", "clamp", "noise", "sampler",
                       "sigma_schedule", "trace"]
    assert (p["timesteps"].default, p["clamp"].default) == (100, False)
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("noise", "sampler", "sigma_schedule", "trace"))
    q = inspect.signature(M.QMDiffusion.refine_tokens).parameters
    assert list(q) == ["self", "sequences", "device", "draft_tokens", "start_step", "strength", "cond_scale", "timesteps", "noise",
                       "sampler", "sigma_schedule", "return_sample"]
    assert all(q[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(q)[5:])
    assert (q["start_step"].default, q["strength"].default, q["timesteps"].default, q["return_sample"].default) == (None, None, 100, False)
    assert M.QMDiffusionForward.refine_tokens is M.QMDiffusion.refine_tokens and M.QMDiffusionForward.refine is M.QMDiffusion.refine
    assert list(inspect.signature(M.strength_sweep).parameters)[:5] == ["model", "sequences", "draft_tokens", "strengths", "device"]
    r = inspect.signature(D.run_refine).parameters
    assert list(r)[:9] == ["engine", "embedding", "pred_dim", "num_steps", "noise", "schedule", "sampler", "sigma_data", "start"]
    assert all(r[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(r)[9:]) and {"source", "draft"} <= set(r)
    from moleculediffusiontransformer_amd.distributed import refine_tokens_sharded
    assert list(inspect.signature(refine_tokens_sharded).parameters) == [
        "local_refine_tokens", "sequences", "draft_tokens", "start_step", "vocab", "group", "model", "guided"]


def test_argument_errors_come_before_anything_is_launched():
    m = tiny()
    seq, draft, src = torch.zeros(3, 12), torch.zeros(3, 32, dtype=torch.long), torch.zeros(3, 16, 32)
    # (no GPU here: anything that got as far as the embedding would raise a RuntimeError instead)
    for start in (2.0, True, [1, 2], [1, 2, 9], 7, -1, [1.0, 2.0, 3.0], None):
        with pytest.raises(ValueError, match="start_step"):
            m.refine(seq, "cuda:0", src, start, timesteps=8)
    for start in (2.0, True, [1, 2], [1, 2, 9], 7, -1, [1.0, 2.0, 3.0]):
        with pytest.raises(ValueError, match="start_step"):
            m.refine_tokens(seq, "cuda:0", draft, start, timesteps=8)
    for strength in (0.0, 1.5, True, [0.5, 0.0, 1.0], [0.5, 0.5]):
        with pytest.raises(ValueError, match="strength"):
            m.refine_tokens(seq, "cuda:0", draft, strength=strength, timesteps=8)
    with pytest.raises(ValueError, match="exactly one of start_step and strength"):
        m.refine_tokens(seq, "cuda:0", draft, timesteps=8)
    with pytest.raises(ValueError, match="exactly one of start_step and strength"):
        m.refine_tokens(seq, "cuda:0", draft, 3, strength=0.5, timesteps=8)
    with pytest.raises(ValueError, match="timesteps"):
        m.refine_tokens(seq, "cuda:0", draft, 0, timesteps=1)
    for d, what in ((draft.float(), "integer"), (draft.bool(), "integer"), (draft[:, :31], r"\(3, 32\)"), (draft[:2], r"\(3, 32\)"),
                    (draft + 16, "pred_dim"), (draft - 1, "pred_dim")):
        with pytest.raises(ValueError, match=what):
            m.refine_tokens(seq, "cuda:0", d, 3, timesteps=8)
    for s in (src.long(), src[:, :15], src[:2]):
        with pytest.raises(ValueError, match="source"):
            m.refine(seq, "cuda:0", s, 3, timesteps=8)
    with pytest.raises(ValueError, match="cond_scale"):
        m.refine_tokens(seq, "cuda:0", draft, 3, cond_scale=[1.0, 2.0], timesteps=8)

    # a sampler without a fused kind: a foreign Sampler, and one of the three classes with its own step()
    class Own(D.ADPM2Sampler):
        def step(self, x, fn, sigma, sigma_next, **k):
            return x
    for smp in (D.Sampler(), Own()):
        with pytest.raises(TypeError, match="needs the fused loop"):
            m.refine_tokens(seq, "cuda:0", draft, 3, timesteps=8, sampler=smp)
        with pytest.raises(TypeError, match="needs the fused loop"):
            m.refine(seq, "cuda:0", src, 3, timesteps=8, sampler=smp)
    # an empty batch: empty results, on any device
    tok, x = m.refine_tokens(seq[:0], "cpu", draft[:0], 3, timesteps=8, return_sample=True)
    assert tok.shape == (0, 32) and tok.dtype == torch.int64 and x.shape == (0, 16, 32) and x.dtype == torch.float32
    assert m.refine_tokens(seq[:0], "cpu", draft[:0], strength=0.5, timesteps=8).shape == (0, 32)
    assert m.refine(seq[:0], "cpu", src[:0], 3, timesteps=8).shape == (0, 16, 32)


# ---------------------------------------------------------------------------------------------------------------------
# the loop on a recording library: which kernels are launched, in which order, with which step / draw / time row
# ---------------------------------------------------------------------------------------------------------------------
class Recorder:
    """Stands for libmdt_hip.so and for the engine: every launch and every evaluation is appended to ``log``."""
    device, has_dual = None, False

    class c:
        in_pad, length, dual_multiple = 16, 32, 1

    def __init__(self):
        self.log, self.times, self.xin = [], None, None

    def __getattr__(self, name):
        if not name.startswith("mdt_"):
            raise AttributeError(name)
        return lambda *a: self.log.append((name,) + a) or 0

    def handoff_check(self, *a, **k):
        pass

    note_handoff = handoff_check
    prepare_context = handoff_check

    def reserve(self, B):
        self.xin, self.pred = torch.zeros(B, 32, 16), torch.zeros(B, 32, 16)

    def prepare_times(self, t):
        self.times = t.clone()

    def select_time(self, row):
        self.log.append(("time", row))

    def eval(self, uncond=False, dual=False):
        self.log.append(("eval", uncond))
        return self.pred


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(rt, "load_library", lambda *a, **k: r)
    monkeypatch.setattr(rt, "current_stream", lambda: 0)
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    return r


def names(log):
    return [e[0] for e in log if e[0].startswith("mdt_")]


SAMPLERS = {"adpm2": lambda: D.ADPM2Sampler(rho=1), "aeuler": D.AEulerSampler, "karras": lambda: D.KarrasSampler(0.05, 5.0, 40.0, 1.003)}
# the update kernels of one step, and the argument index of the draw's index ("step") in the kernel that takes the step's draw
STEP = {"adpm2": (["mdt_adpm2_mid", "mdt_adpm2_next"], "mdt_adpm2_next", 12),
        "aeuler": (["mdt_aeuler_next"], "mdt_aeuler_next", 11),
        "karras": (["mdt_karras_hat", "mdt_karras_mid", "mdt_karras_next"], "mdt_karras_hat", 8)}


@pytest.mark.parametrize("kind", list(SAMPLERS))
def test_run_sampler_keeps_its_launches(rec, kind):
    """The refactoring of _Loop and the step functions (a first step, a per-step hook) leaves run_sampler's launch sequence as it
    was: the first draw, the first input scaling (Karras: none, its churn kernel writes the input), the step's kernels T - 1 times."""
    T, B = 5, 3
    asked = []
    ns = D.NoiseSource(init=torch.zeros(B, 16, 32), steps=lambda i: asked.append(i) or torch.zeros(B, 16, 32))
    tok = torch.zeros(B, 32, dtype=torch.int32)
    D.run_sampler(rec, torch.zeros(B, 12, 128), 16, T, ns, SCHEDULE, SAMPLERS[kind](), 0.1, tokens=tok)
    per_step, drawer, at = STEP[kind]
    head = ["mdt_init_noise"] + ([] if kind == "karras" else ["mdt_precond_in"])
    assert names(rec.log) == head + per_step * (T - 1)
    assert asked == list(range(T - 1))
    assert [e[at + 1] for e in rec.log if e[0] == drawer] == list(range(1, T))          # step i takes draw i + 1
    evals = 1 if kind == "aeuler" else 2
    assert [e[1] for e in rec.log if e[0] == "time"] == list(range(evals * (T - 1)))
    assert "mdt_refine_enter" not in names(rec.log)


@pytest.mark.parametrize("kind", list(SAMPLERS))
@pytest.mark.parametrize("start", [2, [3, 1, 3, 5]])
def test_run_refine_launches(rec, kind, start):
    """Plan and time table of the full T-step call; steps min(start) .. T - 2 only; mdt_refine_enter in front of every step that
    occurs in start (for Karras in front of mdt_karras_hat), with draw 0; step i takes draw i + 1; no draw is asked below min(start)."""
    T, B = 8, 4
    sampler = SAMPLERS[kind]()
    asked = []
    init = torch.zeros(B, 16, 32)
    ns = D.NoiseSource(init=init, steps=lambda i: asked.append(i) or torch.zeros(B, 16, 32))
    draft = torch.zeros(B, 32, dtype=torch.long)
    tok = torch.zeros(B, 32, dtype=torch.int32)
    x = D.run_refine(rec, torch.zeros(B, 12, 128), 16, T, ns, SCHEDULE, sampler, 0.1, start, draft=draft, tokens=tok)
    assert x.shape == (B, 16, 32) and not bool(x.any())               # the state starts zero-filled (nothing ran here)
    sigmas, steps = D.FUSED_SAMPLERS[kind].plan(T, SCHEDULE, sampler, 0.1)
    assert len(steps) == T - 1
    assert torch.equal(rec.times, torch.tensor(D.plan_time_rows(steps), dtype=torch.float32))      # the full call's time table
    starts = [start] * B if isinstance(start, int) else start
    kmin = min(starts)
    per_step, drawer, at = STEP[kind]
    want = []
    for i in range(kmin, T - 1):
        want += (["mdt_refine_enter"] if i in starts else []) + per_step
    assert names(rec.log) == want                                     # no mdt_init_noise, no first mdt_precond_in
    assert asked == list(range(kmin, T - 1))                          # draws 1 .. kmin are never taken
    assert [e[at + 1] for e in rec.log if e[0] == drawer] == list(range(kmin + 1, T))
    evals = 1 if kind == "aeuler" else 2
    assert [e[1] for e in rec.log if e[0] == "time"] == list(range(evals * kmin, evals * (T - 1)))  # a step keeps its time rows
    enters = [e for e in rec.log if e[0] == "mdt_refine_enter"]
    assert [e[4] for e in enters] == sorted(set(starts))
    for e in enters:
        i = e[4]
        s = steps[i]
        assert e[5] == 0 and e[6] != 0 and e[7] == init.data_ptr()    # token form, explicit entry noise
        assert e[8] == float(sigmas[i]) and e[9] == (s.w_hat if kind == "karras" else s.w).c_in
        assert e[11] == 0 and tuple(e[13:17]) == (B, 16, 32, 16)      # draw 0; (B, C, L, Cp)
    # the decode rides in the last update kernel, as in run_sampler
    last = [e for e in rec.log if e[0] == per_step[-1]][-1]
    assert tok.data_ptr() in last


def test_run_refine_refusals(rec):
    emb, draft, src = torch.zeros(3, 12, 128), torch.zeros(3, 32, dtype=torch.long), torch.zeros(3, 16, 32)
    args = (rec, emb, 16, 8, D.NoiseSource(seed=1), SCHEDULE, D.ADPM2Sampler(rho=1), 0.1)
    with pytest.raises(ValueError, match="either dense"):
        D.run_refine(*args, 3)
    with pytest.raises(ValueError, match="either dense"):
        D.run_refine(*args, 3, source=src, draft=draft)
    with pytest.raises(ValueError, match="start"):
        D.run_refine(*args, 7, draft=draft)
    with pytest.raises(ValueError, match="source"):
        D.run_refine(*args, 3, source=src[:, :15])
    with pytest.raises(ValueError, match="draft"):
        D.run_refine(*args, 3, draft=draft.float())
    ns = D.NoiseSource(seed=1)
    ns.init = torch.zeros(3, 16, 31)
    with pytest.raises(ValueError, match="entry noise"):
        D.run_refine(rec, emb, 16, 8, ns, SCHEDULE, D.ADPM2Sampler(rho=1), 0.1, 3, draft=draft)
    with pytest.raises(TypeError, match="no fused loop"):
        D.run_refine(rec, emb, 16, 8, D.NoiseSource(seed=1), SCHEDULE, D.Sampler(), 0.1, 3, draft=draft)
    assert rec.log == []                                              # all of it before anything is launched


def test_header_and_binding_know_the_entry():
    lib = rt.load_library()
    assert hasattr(lib, "mdt_refine_enter") and len(rt.SYMBOLS["mdt_refine_enter"][1]) == 17
    assert lib.mdt_abi_version() == rt.ABI_VERSION == 5               # an addition inside ABI version 5
    # argument checks that need no device: B <= 0 is a no-op; a source given twice / not at all, a null start, L % 4 are refused
    assert lib.mdt_refine_enter(0, 0, 0, 0, 0, 0, 0, 1.0, 1.0, 0, 0, 0, 0, 16, 32, 16, 0) == 0
    assert lib.mdt_refine_enter(8, 8, 8, 0, 0, 0, 0, 1.0, 1.0, 0, 0, 0, 1, 16, 32, 16, 0) != 0
    assert b"dense" in lib.mdt_last_error()
    assert lib.mdt_refine_enter(8, 8, 8, 0, 8, 8, 0, 1.0, 1.0, 0, 0, 0, 1, 16, 32, 16, 0) != 0
    assert lib.mdt_refine_enter(8, 8, 0, 0, 8, 0, 0, 1.0, 1.0, 0, 0, 0, 1, 16, 32, 16, 0) != 0
    assert b"null" in lib.mdt_last_error()
    assert lib.mdt_refine_enter(8, 8, 8, 0, 8, 0, 0, 1.0, 1.0, 0, 0, 0, 1, 16, 30, 16, 0) != 0
    assert lib.mdt_refine_enter(8, 8, 8, 0, 8, 0, 0, 1.0, 1.0, 0, 0, 0, 1, 22, 32, 16, 0) != 0      # Cp < C


def test_refine_tokens_op_schema_and_shape_inference():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from moleculediffusiontransformer_amd import ops  # noqa: F401  (registers torch.ops.mdt.*)
    schema = str(torch.ops.mdt.refine_tokens.default._schema)
    assert schema.startswith("mdt::refine_tokens(Tensor embedding, Tensor draft, Tensor start, Tensor? init_noise, Tensor sigmas, ")
    assert "sampler_kind" in schema and "float[] sampler_params" in schema and schema.endswith("-> (Tensor, Tensor)")
    with FakeTensorMode():
        emb, sig = torch.empty(5, 12, 128), torch.empty(9)
        draft, start = torch.empty(5, 32, dtype=torch.int64), torch.empty(5, dtype=torch.int32)
        x, tok = torch.ops.mdt.refine_tokens(emb, draft, start, None, sig, 1, 22, 0, [1.0], 0.1, 2.0, 7, 0, 0.0)
        assert x.shape == (5, 22, 32) and x.dtype == torch.float32
        assert tok.shape == (5, 32) and tok.dtype == torch.int32
        x, tok = torch.ops.mdt.refine_tokens(emb[:0], draft[:0], start[:0], torch.empty(0, 16, 32), sig, 1, 16, 1, [], 0.1, 1.0, 7, 3)
        assert x.shape == (0, 16, 32) and tok.shape == (0, 32)


# ---------------------------------------------------------------------------------------------------------------------
# the wrappers
# ---------------------------------------------------------------------------------------------------------------------
def test_strength_sweep_is_one_call_of_s_times_b_rows():
    seen = {}

    class Model:
        def refine_tokens(self, seq, device, draft, **k):
            seen.update(seq=seq, device=device, draft=draft, k=k)
            n = seq.shape[0]
            tok = torch.arange(n).view(n, 1).expand(n, 32).clone()
            return (tok, torch.zeros(n, 16, 32)) if k.get("return_sample") else tok
    seq, draft = torch.arange(24.0).view(2, 12), torch.arange(64).view(2, 32) % 16
    tok = M.strength_sweep(Model(), seq, draft, [0.25, 0.5, 1.0], "dev", timesteps=64, cond_scale=2.0)
    assert tok.shape == (3, 2, 32) and tok[:, :, 0].tolist() == [[0, 1], [2, 3], [4, 5]]          # row s * B + b
    assert torch.equal(seen["seq"], seq.repeat(3, 1)) and torch.equal(seen["draft"], draft.repeat(3, 1)) and seen["device"] == "dev"
    assert seen["k"]["start_step"].tolist() == [47, 47, 31, 31, 0, 0] and seen["k"]["cond_scale"] == 2.0
    assert seen["k"]["timesteps"] == 64 and "strength" not in seen["k"]
    tok, x = M.strength_sweep(Model(), seq, draft, (1.0, 0.5), "dev", timesteps=8, return_sample=True)
    assert tok.shape == (2, 2, 32) and x.shape == (2, 2, 16, 32) and seen["k"]["start_step"].tolist() == [0, 0, 3, 3]
    for bad in (0.5, [], [[0.5]], [0.5, 0.0]):
        with pytest.raises(ValueError, match="strength"):
            M.strength_sweep(Model(), seq, draft, bad, "dev", timesteps=8)
    with pytest.raises(ValueError, match="start_step"):
        M.strength_sweep(Model(), seq, draft, [0.5], "dev", timesteps=8, start_step=3)


def test_refine_and_validate_chains_refine_tokens_into_the_forward_model(monkeypatch):
    from moleculediffusiontransformer_amd import generative as G
    seen = {}

    class Inv:
        def refine_tokens(self, *a, **k):
            seen["refine"] = (a, k)
            return torch.full((2, 32), 3)
    monkeypatch.setattr(G, "predict_properties_from_tokens", lambda mf, tok, dev, **k: seen.update(fwd=(mf, tok, dev, k)) or "props")
    cond, draft = torch.zeros(2, 12), torch.ones(2, 32, dtype=torch.long)
    tok, props = M.refine_and_validate(Inv(), "fwd", cond, draft, "cpu", [1, 3], cond_scale=2.0, timesteps=9, forward_timesteps=7,
                                       noise="ns")
    a, k = seen["refine"]
    assert a[0] is cond and a[1] == "cpu" and a[2] is draft and a[3] == [1, 3]
    assert k == dict(strength=None, cond_scale=2.0, timesteps=9, noise="ns", sampler=None, sigma_schedule=None)
    assert props == "props" and seen["fwd"][0] == "fwd" and seen["fwd"][1] is tok
    assert seen["fwd"][3]["timesteps"] == 7 and seen["fwd"][3]["context_embedding_max_length"] == 12


# ---------------------------------------------------------------------------------------------------------------------
# refine_tokens_sharded under gloo, world size 2, uneven shards: a stand-in local function of the GLOBAL sample index
# ---------------------------------------------------------------------------------------------------------------------
def _fake_local_refine(seq, draft, start, first):
    """ids (b, 8) in [0, 16): a function of the global sample index, the conditioning, the draft and the row's own start"""
    b = seq.shape[0]
    idx = torch.arange(first, first + b).view(b, 1)
    st = torch.as_tensor(start).expand(b).view(b, 1) if not isinstance(start, int) else torch.full((b, 1), start)
    return (idx * 5 + torch.arange(8).view(1, 8) * 3 + seq.sum(dim=1, keepdim=True).round().long() + draft + 7 * st) % 16


def _inputs(total):
    seq = torch.arange(total * 4, dtype=torch.float32).view(total, 4) * 0.25
    draft = (torch.arange(total * 8).view(total, 8) * 7) % 16
    start = (torch.arange(total) * 3) % 6
    return seq, draft, start


class _FakeModel:
    def __init__(self):
        self.kernel_choice = "auto"

    def pin_kernel_choice(self, batch):
        self.kernel_choice = None if batch is None else ("wide" if batch > 1024 else "narrow")


def _worker(rank, world, port, total, q):
    from moleculediffusiontransformer_amd.distributed import refine_tokens_sharded, shard_bounds
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        seq, draft, start = _inputs(total)
        m, seen = _FakeModel(), []

        def local(s, d, st, first):
            seen.append((first, s.shape[0], d.shape[0], len(st), m.kernel_choice))         # pinned BEFORE the local call
            return _fake_local_refine(s, d, st, first)
        tok = refine_tokens_sharded(local, seq, draft, start, vocab=16, model=m, guided=True)
        assert tok.dtype == torch.int64
        scalar = refine_tokens_sharded(lambda s, d, st, first: _fake_local_refine(s, d, st, first), seq, draft, 4, vocab=16)
        q.put((rank, tok.numpy(), scalar.numpy(), seen[0], shard_bounds(total, world, rank)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("total", [7, 8])
def test_two_rank_sharded_refine_equals_single_rank(total):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, total, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    seq, draft, start = _inputs(total)
    want, want_scalar = _fake_local_refine(seq, draft, start, 0), _fake_local_refine(seq, draft, 4, 0)
    for rank, tok, scalar, (first, ns, nd, nst, choice), (lo, hi) in results:
        assert torch.equal(torch.from_numpy(tok), want) and torch.equal(torch.from_numpy(scalar), want_scalar), rank
        assert (first, ns, nd, nst) == (lo, hi - lo, hi - lo, hi - lo) and choice == "narrow", rank
    # one rank, no process group: the local result itself; a list of starts is sliced like a tensor
    from moleculediffusiontransformer_amd.distributed import refine_tokens_sharded
    assert torch.equal(refine_tokens_sharded(_fake_local_refine, seq, draft, start, vocab=16), want)
    assert torch.equal(refine_tokens_sharded(_fake_local_refine, seq, draft, start.tolist(), vocab=16), want)
    with pytest.raises(ValueError, match="same"):
        refine_tokens_sharded(_fake_local_refine, seq, draft[:-1], start, vocab=16)
    with pytest.raises(ValueError, match="start_step"):
        refine_tokens_sharded(_fake_local_refine, seq, draft, start[:-1], vocab=16)


# ---------------------------------------------------------------------------------------------------------------------
# the fixture
# ---------------------------------------------------------------------------------------------------------------------
CASES = {"a": ("tiny", "adpm2", 1.0, [4, 4, 4]), "b": ("tiny", "adpm2", 2.0, [3, 3, 3]), "c": ("pd22", "adpm2", 1.0, [4, 4, 4]),
         "d": ("pd22", "adpm2", 2.0, [3, 3, 3]), "e": ("tiny", "aeuler", 2.0, [2, 2, 2]), "f": ("pd22", "aeuler", 1.0, [5, 5, 5]),
         "rows1": ("tiny", "adpm2", 2.0, [1, 3, 5]), "rows2": ("pd22", "adpm2", 1.0, [0, 4, 6])}


def test_fixture_identities():
    g = load_golden("refine.npz")
    assert [str(c) for c in g["cases"]] == list(CASES)
    for (name, (model, sampler, cs, start)), gm, gs, gt in zip(CASES.items(), g["models"], g["samplers"], g["tags"]):
        assert (str(gm), str(gs), str(gt)) == (model, sampler, f"rf_{model}")
        C = {"tiny": 16, "pd22": 22}[model]
        assert g[f"{name}_seq"].shape == (3, 12) and g[f"{name}_draft"].shape == (3, 32) and g[f"{name}_out"].shape == (3, C, 32)
        assert g[f"{name}_out"].dtype == np.float32 and g[f"{name}_tokens"].shape == (3, 32)
        assert g[f"{name}_start"].tolist() == start and int(g[f"{name}_timesteps"]) == 8 and float(g[f"{name}_cond_scale"]) == cs
        assert 0 <= g[f"{name}_draft"].min() and g[f"{name}_draft"].max() < C
        # tokens are the argmax of the sample, and every position's top-two margin is above twice the 1e-4 sample tolerance
        out = torch.from_numpy(g[f"{name}_out"])
        assert torch.equal(out.argmax(dim=1), torch.from_numpy(g[f"{name}_tokens"]))
        top2 = torch.topk(out, 2, dim=1).values
        margin = (top2[:, 0] - top2[:, 1]).flatten(1).min(dim=1).values
        assert torch.equal(margin, torch.from_numpy(g[f"{name}_margin"])) and float(margin.min()) > 2e-4
    # the per-sample cases are stitched from scalar runs: where a scalar case has the same model, scale and start, the rows agree
    assert np.array_equal(g["rows1_out"][1], g["b_out"][1]) and np.array_equal(g["rows2_out"][1], g["c_out"][1])
    assert np.array_equal(g["rows1_draft"], g["b_draft"]) and np.array_equal(g["rows2_seq"], g["c_seq"])
    assert float(g["last_start_margin"]) > 1.9                       # start T - 2 on tiny keeps the draft, with a margin near 2
