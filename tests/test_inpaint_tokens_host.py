"""CPU: the host side of inpaint_tokens() -- one_hot_draft, the fixture recorded from the real reference against the oracle, the
class surface and its argument errors, the two new C ABI entries, the shape inference of mdt::inpaint_tokens, and the sharded
wrapper under gloo."""
import inspect
import os
import re
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

from conftest import ROOT, load_golden
from helpers import oracle_cfg, synth_sd, to_t
import moleculediffusiontransformer_amd as M
from moleculediffusiontransformer_amd import runtime as rt
from moleculediffusiontransformer_amd.synth import synth_normal
from oracle import unet_oracle as O

ORACLE_TOL = 2e-6    # the oracle's bound against the reference (test_oracle_golden.py)


def fixture_cases():
    g = load_golden("inpaint_tokens.npz")
    for name, model, tag in zip(g["cases"], g["models"], g["tags"]):
        yield str(name), str(model), str(tag), {k[len(name) + 1:]: v for k, v in g.items() if k.startswith(f"{name}_")}


def reference_one_hot(tokens, num_classes):
    """encode_SMILES_into_one_hot's tensor half (generative.py:1567-1569) and the permute of its caller (:1603)."""
    oh = F.one_hot(tokens.long(), num_classes=num_classes)
    oh[oh == 0] = -1
    return torch.permute(oh.float(), (0, 2, 1))


def test_one_hot_draft_is_the_reference_recipe_bit_for_bit():
    for C, dtype in ((16, torch.int64), (22, torch.int32), (3, torch.uint8)):
        tok = torch.randint(0, C, (5, 32), generator=torch.Generator().manual_seed(C)).to(dtype)
        got = M.one_hot_draft(tok, C)
        assert got.dtype == torch.float32 and got.shape == (5, C, 32) and got.is_contiguous()
        assert torch.equal(got, reference_one_hot(tok, C))
        assert torch.equal(got.argmax(dim=1), tok.long()) and set(got.unique().tolist()) == {-1.0, 1.0}


def test_fixture_has_the_cases_of_the_generator():
    cases = list(fixture_cases())
    assert [(n, m, t) for n, m, t, _ in cases] == [("a", "tiny", "it_tiny_a"), ("b", "tiny", "it_tiny_b"), ("c", "pd22", "it_pd22")]
    for name, model, tag, g in cases:
        T, R = int(g["timesteps"]), int(g["num_resamples"])
        assert int(g["ndraws"]) == 1 + (T - 1) * 2 * R
        assert g["draft"].shape == g["keep"].shape == g["tokens"].shape == g["out"].shape[::2]
        assert g["keep"].dtype == bool and float(g["margin"]) > 2e-4


@pytest.mark.parametrize("name,model,tag,g", list(fixture_cases()), ids=lambda v: v if isinstance(v, str) else "")
def test_oracle_reproduces_the_fixture(name, model, tag, g):
    """oracle.unet_oracle.adpm2_inpaint on the one-hot draft and the channel-repeated mask: the sample at the oracle's bound, its
    argmax the recorded tokens, the kept region the one-hot draft."""
    sd, cfg = synth_sd(model), oracle_cfg(model)
    draft, keep, out_ref = to_t(g["draft"]), to_t(g["keep"]), to_t(g["out"])
    C = out_ref.shape[1]
    src = M.one_hot_draft(draft, C)
    mask = keep.unsqueeze(1).expand(-1, C, -1)
    n = {"i": 0}

    def draw(like):
        t = synth_normal(f"{tag}/draw{n['i']}", tuple(like.shape))
        n["i"] += 1
        return t
    with torch.no_grad():
        emb = O.cond_embed(sd, cfg, to_t(g["seq"]))
    out = O.adpm2_inpaint(sd, cfg, src, mask, emb, int(g["timesteps"]), int(g["num_resamples"]), draw, float(g["cond_scale"]))
    assert n["i"] == int(g["ndraws"])
    assert (out - out_ref).abs().max() <= ORACLE_TOL
    assert torch.equal(out.argmax(dim=1), to_t(g["tokens"]))
    assert torch.equal(out[mask], src[mask]) and torch.equal(to_t(g["tokens"])[keep], draft[keep])


def test_class_surface():
    p = inspect.signature(M.QMDiffusion.inpaint_tokens).parameters
    assert list(p) == ["self", "sequences", "device", "draft_tokens", "keep_mask", "cond_scale", "timesteps", "num_resamples",
                       "draw", "seed", "sample0", "return_sample"]
    assert (p["cond_scale"].default, p["timesteps"].default, p["num_resamples"].default) == (7.5, 100, 1)
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("draw", "seed", "sample0", "return_sample"))
    assert (p["draw"].default, p["seed"].default, p["sample0"].default, p["return_sample"].default) == (None, None, 0, False)
    assert M.QMDiffusionForward.inpaint_tokens is M.QMDiffusion.inpaint_tokens          # it lives on the common base
    q = inspect.signature(M.QMDiffusion.inpaint).parameters
    assert list(q)[:8] == ["self", "sequences", "device", "cond_scale", "timesteps", "num_resamples", "inpaint", "in_paint_mask"]
    assert q["sample0"].kind is inspect.Parameter.KEYWORD_ONLY and q["sample0"].default == 0
    c = inspect.signature(M.complete_and_validate).parameters
    assert list(c)[:6] == ["model", "model_forward", "conditioning", "draft_tokens", "keep_mask", "device"]
    gv = inspect.signature(M.generate_and_validate).parameters
    for k in ("cond_scale", "timesteps", "forward_timesteps", "X_norm_factor", "forward_noise"):     # generate_and_validate's
        assert c[k].default == gv[k].default and c[k].kind == gv[k].kind
    assert c["num_resamples"].default == 1
    from moleculediffusiontransformer_amd.distributed import inpaint_tokens_sharded
    assert list(inspect.signature(inpaint_tokens_sharded).parameters) == [
        "local_inpaint_tokens", "sequences", "draft_tokens", "keep_mask", "vocab", "group", "model", "guided"]


def test_complete_and_validate_chains_inpaint_tokens_into_the_forward_model(monkeypatch):
    from moleculediffusiontransformer_amd import generative as G
    seen = {}

    class Inv:
        def inpaint_tokens(self, *a, **k):
            seen["inpaint"] = (a, k)
            return torch.full((2, 32), 3)
    monkeypatch.setattr(G, "predict_properties_from_tokens", lambda mf, tok, dev, **k: seen.update(fwd=(mf, tok, dev, k)) or "props")
    cond, draft, keep = torch.zeros(2, 12), torch.ones(2, 32, dtype=torch.long), torch.zeros(2, 32, dtype=torch.bool)
    tok, props = M.complete_and_validate(Inv(), "fwd", cond, draft, keep, "cpu", cond_scale=2.0, timesteps=9, forward_timesteps=7,
                                         num_resamples=3, seed=5, sample0=4)
    a, k = seen["inpaint"]
    assert a[0] is cond and a[1] == "cpu" and a[2] is draft and a[3] is keep
    assert k == dict(cond_scale=2.0, timesteps=9, num_resamples=3, draw=None, seed=5, sample0=4)
    assert props == "props" and seen["fwd"][0] == "fwd" and seen["fwd"][1] is tok
    assert seen["fwd"][3]["timesteps"] == 7 and seen["fwd"][3]["context_embedding_max_length"] == 12


def test_argument_errors():
    m = M.QMDiffusion(max_length=32, pred_dim=16, channels=16, context_embedding_max_length=12, text_embed_dim=64,
                      embed_dim_position=64)
    seq = torch.zeros(3, 12)
    draft, keep = torch.zeros(3, 32, dtype=torch.long), torch.zeros(3, 32, dtype=torch.bool)
    bad = [(draft.float(), keep, "integer"), (draft.bool(), keep, "integer"), (draft, keep.long(), "bool"),
           (draft[:, :31], keep[:, :31], r"\(3, 32\)"), (draft[:2], keep[:2], r"\(3, 32\)"), (draft, keep[:, :16], r"\(3, 32\)"),
           (draft.view(3, 32, 1), keep, r"\(3, 32\)"), (draft + 16, keep, "pred_dim"), (draft - 1, keep, "pred_dim")]
    for d, k, what in bad:
        with pytest.raises(ValueError, match=what):
            m.inpaint_tokens(seq, "cuda:0", d, k, timesteps=4, seed=1)
    tok, x = m.inpaint_tokens(seq[:0], "cpu", draft[:0], keep[:0], return_sample=True)     # an empty batch: empty results
    assert tok.shape == (0, 32) and tok.dtype == torch.int64 and x.shape == (0, 16, 32) and x.dtype == torch.float32
    assert m.inpaint_tokens(seq[:0], "cpu", draft[:0], keep[:0]).shape == (0, 32)
    # the loop itself refuses a source given twice, or half a token form
    from moleculediffusiontransformer_amd.diffusion import ADPM2Sampler, KarrasSchedule, run_adpm2_inpaint
    args = (4, 1, None, 1, KarrasSchedule(0.001, 9.0, 3.0), ADPM2Sampler(rho=1), 0.1)

    class Eng:
        device = "cpu"
    with pytest.raises(ValueError, match="either dense"):
        run_adpm2_inpaint(Eng(), None, torch.zeros(3, 16, 32), torch.zeros(3, 16, 32, dtype=torch.bool), *args, draft=draft, keep=keep)
    with pytest.raises(ValueError, match="same shape"):
        run_adpm2_inpaint(Eng(), None, torch.zeros(3, 16, 32), torch.zeros(3, 32, dtype=torch.bool), *args)
    with pytest.raises(ValueError, match="pred_dim"):
        run_adpm2_inpaint(Eng(), None, None, None, *args, draft=draft, keep=keep)
    with pytest.raises(ValueError, match="bool"):
        run_adpm2_inpaint(Eng(), None, None, None, *args, draft=draft, keep=keep.long(), pred_dim=16)


def test_header_declares_and_binding_knows_the_new_entries():
    hdr = open(os.path.join(ROOT, "include", "mdt_hip.h")).read()
    for name, nargs in (("mdt_inpaint_enter", 20), ("mdt_inpaint_finish", 10)):
        decl = re.search(rf"\bint {name}\s*\(([^;]*)\);", hdr)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == nargs == len(rt.SYMBOLS[name][1])
    lib = rt.load_library()
    assert hasattr(lib, "mdt_inpaint_enter") and hasattr(lib, "mdt_inpaint_finish")
    assert lib.mdt_abi_version() == rt.ABI_VERSION == 5              # additions inside ABI version 5
    for name in ("mdt_inpaint_merge", "mdt_add_noise", "mdt_precond_in", "mdt_argmax_tokens"):      # what they fuse stays exported
        assert hasattr(lib, name) and name in rt.SYMBOLS
    # argument checks that need no device: B <= 0 is a no-op, a source given twice / not at all is refused
    assert lib.mdt_inpaint_enter(0, 0, 0, 0, 0, 0, 0, 0, 1.0, 0.0, 1.0, 0, 0, 0, 0, 0, 16, 32, 16, 0) == 0
    assert lib.mdt_inpaint_finish(0, 0, 0, 0, 0, 0, 0, 16, 32, 0) == 0
    assert lib.mdt_inpaint_enter(8, 8, 0, 0, 8, 0, 0, 0, 1.0, 0.0, 1.0, 0, 0, 0, 0, 1, 16, 32, 16, 0) != 0
    assert b"dense" in lib.mdt_last_error()
    assert lib.mdt_inpaint_finish(8, 8, 8, 8, 0, 0, 1, 16, 32, 0) != 0
    assert lib.mdt_inpaint_enter(8, 8, 8, 0, 8, 0, 0, 0, 1.0, 0.0, 1.0, 0, 0, 0, 0, 1, 16, 30, 16, 0) != 0      # L % 4


def test_inpaint_tokens_op_shape_inference():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from moleculediffusiontransformer_amd import ops  # noqa: F401  (registers torch.ops.mdt.*)
    with FakeTensorMode():
        emb, sig = torch.empty(5, 12, 128), torch.empty(9)
        draft, keep = torch.empty(5, 32, dtype=torch.int64), torch.empty(5, 32, dtype=torch.bool)
        x, tok = torch.ops.mdt.inpaint_tokens(emb, draft, keep, sig, 1, 22, 2, 1.0, 0.1, 2.0, 7, 0, 0.0)
        assert x.shape == (5, 22, 32) and x.dtype == torch.float32
        assert tok.shape == (5, 32) and tok.dtype == torch.int32
        x, tok = torch.ops.mdt.inpaint_tokens(emb[:0], draft[:0], keep[:0], sig, 1, 16, 1, 1.0, 0.1, 1.0, 7, 3)
        assert x.shape == (0, 16, 32) and tok.shape == (0, 32)


# ---------------------------------------------------------------------------------------------------------------------
# inpaint_tokens_sharded under gloo, world size 2, uneven shards: a stand-in local function of the GLOBAL sample index
# ---------------------------------------------------------------------------------------------------------------------
def _fake_local_inpaint(seq, draft, keep, first):
    """ids (b, 8) in [0, 16): the draft where kept, else a function of the global sample index and the conditioning"""
    b = seq.shape[0]
    idx = torch.arange(first, first + b).view(b, 1)
    gen = (idx * 5 + torch.arange(8).view(1, 8) * 3 + seq.sum(dim=1, keepdim=True).round().long()) % 16
    return torch.where(keep, draft, gen)


def _inputs(total):
    seq = torch.arange(total * 4, dtype=torch.float32).view(total, 4) * 0.25
    draft = (torch.arange(total * 8).view(total, 8) * 7) % 16
    keep = (torch.arange(total * 8).view(total, 8) % 3) == 0
    return seq, draft, keep


class _FakeModel:
    def __init__(self):
        self.kernel_choice = "auto"

    def pin_kernel_choice(self, batch):
        self.kernel_choice = None if batch is None else ("wide" if batch > 1024 else "narrow")


def _worker(rank, world, port, total, q):
    from moleculediffusiontransformer_amd.distributed import inpaint_tokens_sharded, shard_bounds
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        seq, draft, keep = _inputs(total)
        m, seen = _FakeModel(), []

        def local(s, d, k, first):
            seen.append((first, s.shape[0], d.shape[0], k.shape[0], m.kernel_choice))      # pinned BEFORE the local call
            return _fake_local_inpaint(s, d, k, first)
        tok = inpaint_tokens_sharded(local, seq, draft, keep, vocab=16, model=m, guided=True)
        assert tok.dtype == torch.int64
        q.put((rank, tok.numpy(), seen[0], shard_bounds(total, world, rank)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("total", [7, 8])
def test_two_rank_sharded_completion_equals_single_rank(total):
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
    seq, draft, keep = _inputs(total)
    want = _fake_local_inpaint(seq, draft, keep, 0)
    assert torch.equal(want[keep], draft[keep])
    for rank, tok, (first, ns, nd, nk, choice), (lo, hi) in results:
        assert torch.equal(torch.from_numpy(tok), want), rank
        assert (first, ns, nd, nk) == (lo, hi - lo, hi - lo, hi - lo) and choice == "narrow", rank
    # one rank, no process group: the local result itself
    from moleculediffusiontransformer_amd.distributed import inpaint_tokens_sharded
    assert torch.equal(inpaint_tokens_sharded(_fake_local_inpaint, seq, draft, keep, vocab=16), want)
    with pytest.raises(ValueError, match="same"):
        inpaint_tokens_sharded(_fake_local_inpaint, seq, draft[:-1], keep, vocab=16)
