"""k_tf256's loader turn on the GPU (the whole-tile schedule the library ships, and -- in a tuning build with -DMDT_RING_HALF=1 --
the half-ahead schedule of csrc/mdt_ring_sched.h; both passed this file when it was written): single MDT_OP_TF256 ops through the
C ABI against the CPU interpreter (oracle/program_interp.py) at the tolerances of tests/test_gpu_ops.py::test_fused_transformer,
over the streams that change which tiles are first, last, whole or split -- and ten launches per case on the same inputs, which
must agree bit for bit: a tile published before it landed (the counted wait is rounded, the allowance has three terms), or refilled
while a fragment read was in flight, shows as a difference between launches before it shows against the reference."""
import pytest
import torch

from moleculediffusiontransformer_amd import runtime as rt
from oracle.program_interp import Buffers, run_program

from gpu_util import DEV, ref, rnd
from test_gpu_ops import _handoff_ext, _transformer_sd

pytestmark = pytest.mark.gpu
A, S = rt.SP_ACT, rt.SP_SHR
C, T, N_CTX, MID = 256, 4, 12, 512
REPEATS = 10


def _build(layers, cross, form, prod, in_out):
    """One MDT_OP_TF256 (8 heads, 8 hidden chunks) and its packed weights.  in_out False: the op WITHOUT to_in and the folded
    closing convolution (MDT_F_HAS_IN = MDT_F_NPOST = 0) -- the descriptor tables lose the to_in sub-block in front and the
    convolution's output tiles at the end, the vectors their first sub-block, every vector descriptor counts one sub-block less:
    the first tiles of the launch are then a self-attention head's, the last weight tile a feed-forward output tile."""
    from moleculediffusiontransformer_amd.compiler import Ten, UNetCompiler
    from moleculediffusiontransformer_amd.netspec import inverse_unet_config
    cfg = inverse_unet_config(16, 64, 128, N_CTX)
    sd = _transformer_sd("tf.", C, layers, cross)
    comp = UNetCompiler(cfg, 64, N_CTX, sd, gemm_mode=prod, tf256=(form == "wide"))
    comp.transformer(Ten(A, 0, T, C), "tf.", C, layers, cross, free_input=False)
    assert [o.kind for o in comp.ops] == [rt.OP_TF256]
    op = comp.ops[0]
    assert op.i[rt.F_WF32] == int(prod == "f32") and op.i[rt.F_NSPLIT] == (1 if form == "wide" else 2)
    assert op.i[rt.F_HEADS] == 8 and op.i[rt.F_NFF] == 8
    op.out = ref(A, T * C)
    if cross:
        op.a2 = ref(A, 2 * T * C)
    W = comp.W.pack()
    if not in_out:
        nt, nsplit = op.i[rt.F_NT], op.i[rt.F_NSPLIT]
        words = W[op.p0.off: op.p0.off + nsplit * nt].contiguous().view(torch.int32).tolist()
        n_in, n_scr, n_post = (C // 64) * 2 // nsplit, 2 * nsplit, op.i[rt.F_NPOST] // nsplit
        tabs = []
        for hh in range(nsplit):
            t = words[hh * nt: (hh + 1) * nt]
            assert all(w & 7 == 0 for w in t[:n_in]) and t[n_in] & 7 == 5 and all(w & 7 == 4 for w in t[n_in + 1: n_in + n_scr])
            assert all(w & 7 == 1 for w in t[nt - n_scr - n_post: nt - n_scr]) and all(w & 7 == 4 for w in t[nt - n_scr:])
            t = t[n_in + n_scr: nt - n_scr - n_post] + t[nt - n_scr:]
            for k, w in enumerate(t):
                if w & 7 == 5:                                 # vectors of sub-block nxt -> nxt - 1
                    nxt = (w >> 4) // 3 - 1
                    t[k] = 5 | ((3 * nxt) << 1 | (nxt & 1)) << 3
            tabs.append(t)
        nt2 = len(tabs[0])
        W[op.p0.off: op.p0.off + nsplit * nt2] = torch.tensor([w for t in tabs for w in t], dtype=torch.int32).view(torch.float32)
        op.bias = rt.MdtRef(op.bias.space, 0, op.bias.off + 768)
        op.i[rt.F_NT], op.i[rt.F_NVEC], op.i[rt.F_HAS_IN], op.i[rt.F_NPOST] = nt2, op.i[rt.F_NVEC] - 768, 0, 0
    return op, W


def _check(op, W, B, layers, cross, form, kv2=False, occupy=False):
    kv_floats = N_CTX * 2 * MID
    act = torch.cat([rnd(B * T * C, seed=13) * 1.5 + 0.3, torch.zeros(B * T * C), rnd(layers * B * kv_floats, seed=14) if cross else torch.zeros(0)])
    shr = rnd(layers * kv_floats, seed=15) if kv2 else torch.zeros(4)
    ext = _handoff_ext(B, T) if form == "narrow" else {}
    cpu = Buffers(W.clone(), act.clone(), shr.clone(), {k: v.clone().view(-1) for k, v in ext.items()})
    run_program([op], cpu, B, 0)
    want = cpu.act[B * T * C: 2 * B * T * C]
    gw, ga, gs = W.to(DEV), act.to(DEV), shr.to(DEV)
    ge = {k: v.to(DEV) for k, v in ext.items()}
    b = rt.MdtBindings()
    b.weights, b.act, b.shr = rt.ptr(gw), rt.ptr(ga), rt.ptr(gs)
    for k, v in ge.items():
        b.ext[k] = rt.ptr(v)
    prog = rt.Program([op])
    lib = rt.load_library()
    outs = []
    with torch.cuda.device(DEV):
        side = torch.cuda.Stream(device=DEV) if occupy else None
        for rep in range(REPEATS):
            ga[B * T * C: 2 * B * T * C].zero_()
            if occupy:          # part of the device held on a second stream while the launch runs (tools/stress_chain_uneven.py)
                torch.cuda.synchronize()
                rt.check(lib.mdt_test_occupy((37 * rep) % 200 + 8, 160 * 1024, 30000, side.cuda_stream))
            prog.run(b, B, 0)
            outs.append(ga[B * T * C: 2 * B * T * C].clone())
        torch.cuda.synchronize()
    got = [o.cpu() for o in outs]
    assert torch.isfinite(got[0]).all()
    for rep, o in enumerate(got[1:], 1):
        assert torch.equal(o, got[0]), f"launch {rep} differs from launch 0 on the same inputs"
    if ext:
        flags = ge[3].view(torch.int32).cpu()
        nsub = int(bool(op.i[rt.F_HAS_IN])) + layers * (3 if cross else 2)
        assert int(flags[0]) == 0, "a hand-off poll timed out"
        assert bool((flags[64::32] == REPEATS * nsub).all())
    tol = 2e-4 * max(1.0, want.abs().max().item())
    err = (got[0] - want).abs().max().item()
    assert err < tol, (err, tol)
    assert torch.equal(ga[: B * T * C].cpu(), act[: B * T * C])                       # inputs untouched


@pytest.mark.parametrize("prod", ["bf16x3", "f32"])
@pytest.mark.parametrize("form", ["narrow", "wide"])
@pytest.mark.parametrize("in_out", [True, False], ids=["in_out", "bare"])
@pytest.mark.parametrize("cross", [False, True], ids=["self", "cross"])
@pytest.mark.parametrize("layers", [1, 2])
def test_tf256_streams(layers, cross, in_out, form, prod):
    """8 samples = one 32-row block, 9 = a ragged second block, 24 = three blocks; every case ten times, bit for bit."""
    op, W = _build(layers, cross, form, prod, in_out)
    for B in (8, 9, 24):
        _check(op, W, B, layers, cross, form)


@pytest.mark.parametrize("prod", ["bf16x3", "f32"])
@pytest.mark.parametrize("form", ["narrow", "wide"])
def test_tf256_dual_batch(form, prod):
    """The dual-batch form (MDT_F_KV2): the second half of the batch reads shared K / V rows."""
    op, W = _build(2, True, form, prod, True)
    op.p1 = ref(S, 0)
    op.i[rt.F_KV2] = 1
    _check(op, W, 16, 2, True, form, kv2=True)


def test_tf256_under_uneven_load():
    """Ten launches of the pair-split form while mdt_test_occupy holds a varying part of the device on a second stream: the
    same bits, and the hand-off's status word stays 0."""
    op, W = _build(2, True, "narrow", "bf16x3", True)
    _check(op, W, 24, 2, True, "narrow", occupy=True)
