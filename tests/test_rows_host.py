"""CPU tests of the per-row evaluation form (one noise level per sample): the compiled programs, the FiLM batch stride in the op
encoding, the per-sample coefficient helper, the class surface without a GPU."""
import inspect

import numpy as np
import pytest
import torch

from conftest import load_golden
from moleculediffusiontransformer_amd import QMDiffusion, QMDiffusionForward, runtime as rt
from moleculediffusiontransformer_amd.compiler import EXT_FILM, compile_unet
from moleculediffusiontransformer_amd.diffusion import scale_weights, scale_weights_rows
from moleculediffusiontransformer_amd.synth import make_synth_model

FILM_KINDS = (rt.OP_GEMM, rt.OP_GN_ACT, rt.OP_RCONV, rt.OP_RESBLOCK, rt.OP_PREP16, rt.OP_TF128, rt.OP_RES256)


def _compiled(case, mode, rows):
    m = make_synth_model(case)
    sd = {k: v.detach().float().cpu() for k, v in m.unet.state_dict().items()}
    return compile_unet(m.unet.config, m.max_length, m.unet.config.ctx_max_length, sd, gemm_mode=mode, rows=rows)


def _reads_film(op, c):
    """Does the op read FiLM rows of the time mapping (p3 inside the shared ss_cur row or the per-sample table)?"""
    if op.kind not in FILM_KINDS or op.p3.space == rt.SP_NONE:
        return False
    if op.p3.space == rt.SP_EXT0 + EXT_FILM:
        return True
    return op.p3.space == rt.SP_SHR and c.shr["ss_cur"] <= op.p3.off < c.shr["ss_cur"] + c.ss_total


@pytest.mark.parametrize("mode", ["bf16x3", "f32"])
@pytest.mark.parametrize("case", ["tiny", "cfg1"])
def test_per_row_program_binds_every_film_consumer_with_a_batch_stride(case, mode):
    c = _compiled(case, mode, rows=True)
    assert c.rows and set(c.programs) == {"time_rows", "ctx", "ctx_fixed", "eval_rows", "eval_rows_fixed"}
    for name in ("eval_rows", "eval_rows_fixed"):
        ops = c.programs[name]
        film = [op for op in ops if _reads_film(op, c)]
        assert len(film) == 18                                           # one per ResnetBlock1d
        for op in film:
            assert op.p3.space == rt.SP_EXT0 + EXT_FILM and op.film_bstride == c.ss_total and op.film_bstride % 4 == 0
            width = {rt.OP_GN_ACT: rt.N_LD, rt.OP_GEMM: rt.G_CIN, rt.OP_RCONV: rt.R_C, rt.OP_RESBLOCK: rt.K_COUT}[op.kind]
            assert op.p3.off + 2 * op.i[width] <= c.ss_total
        # nothing reads the shared arena's time tables: the per-row form has none
        assert not any(op.p3.space == rt.SP_SHR and op.kind in FILM_KINDS for op in ops)
        assert all(op.film_bstride == 0 for op in ops if op not in film)
        rt.Program(ops)                                                  # the library's validation accepts the encoding
    assert c.max_time_rows == 0 and "c_noise" in c.act_named
    # the time program runs one row per sample (M_MODE 0) into the per-sample table
    time = c.programs["time_rows"]
    assert all(op.i[rt.G_M_MODE] == 0 for op in time if op.kind == rt.OP_GEMM)
    assert time[-1].out.space == rt.SP_EXT0 + EXT_FILM and time[-1].i[rt.G_N] == c.ss_total
    rt.Program(time)
    if case == "cfg1":
        kinds = [op.kind for op in c.programs["eval_rows"]]
        assert rt.OP_ATTN not in kinds and rt.OP_TBLOCK not in kinds
        assert kinds.count(rt.OP_TF128) == 4 and kinds.count(rt.OP_TF256) == 5
        assert len(kinds) == 63                                   # k_rconv and k_resblock take the stride: 103 -> 71 -> 63
        assert kinds.count(rt.OP_RESBLOCK) == 2 and kinds.count(rt.OP_RCONV) == 52
        # every Transformer1d launch is transformer-only: the ResNet chains of k_tf128 / k_res256 stage one shared FiLM row
        assert all(op.i[rt.F_N_RES] == 0 for op in c.programs["eval_rows"] if op.kind == rt.OP_TF128)
        assert rt.OP_RES256 not in kinds
        if mode == "f32":
            wf = {rt.OP_TF128: rt.F_WF32, rt.OP_TF256: rt.F_WF32, rt.OP_RCONV: rt.R_WF32}
            assert all(op.i[wf[op.kind]] == 1 for op in c.programs["eval_rows"] if op.kind in wf)


@pytest.mark.parametrize("mode", ["bf16x3", "f32"])
@pytest.mark.parametrize("case", ["tiny", "cfg1"])
def test_default_programs_keep_stride_zero(case, mode):
    c = _compiled(case, mode, rows=False)
    assert not c.rows and "eval_rows" not in c.programs and "time" in c.programs
    for name, ops in c.programs.items():
        assert all(op.film_bstride == 0 for op in ops), name
    assert sum(_reads_film(op, c) for op in c.programs["eval"]) > 0
    assert not any(op.p3.space == rt.SP_EXT0 + EXT_FILM for op in c.programs["eval"])


@pytest.mark.parametrize("case", ["pd22", "cfg3", "nb", "sparse", "full"])
def test_per_row_program_compiles_for_every_model_shape(case):
    """Blocks outside k_resblock / k_rconv's shapes run as GroupNorm passes + GEMMs; those with a channel count that is not a
    multiple of 16 (pred_dim 22 / 3) take the GroupNorm prologue of MDT_OP_GEMM: it carries the stride too."""
    c = _compiled(case, "bf16x3", rows=True)
    film = [op for op in c.programs["eval_rows"] if op.p3.space == rt.SP_EXT0 + EXT_FILM]
    assert film and all(op.film_bstride == c.ss_total for op in film)
    assert {op.kind for op in film} <= {rt.OP_GN_ACT, rt.OP_GEMM, rt.OP_RCONV, rt.OP_RESBLOCK}
    if case in ("pd22", "sparse"):
        assert any(op.kind == rt.OP_GEMM for op in film)
    rt.Program(c.programs["eval_rows"])


def test_plain_bf16_mode_refuses_the_per_row_form():
    with pytest.raises(ValueError, match="bf16x3.*f32"):
        _compiled("tiny", "bf16", rows=True)


def test_library_refuses_a_stride_on_ops_that_read_one_shared_row():
    c = _compiled("cfg1", "bf16x3", rows=False)
    op = next(o for o in c.programs["eval"] if o.kind == rt.OP_TF128 and o.i[rt.F_N_RES] > 0)      # a chain: one row per block
    bad = rt.MdtOp()
    import ctypes
    ctypes.memmove(ctypes.byref(bad), ctypes.byref(op), ctypes.sizeof(rt.MdtOp))
    bad.film_bstride = c.ss_total
    with pytest.raises(RuntimeError, match="film_bstride"):
        rt.Program([bad])


def test_per_sample_coefficients_equal_the_scalar_helper_bit_for_bit():
    g = load_golden("scalars.npz")
    sig = torch.from_numpy(g["sigmas_64"])
    sig = sig[sig != 0]
    assert sig.numel() == 64
    for n in (64, 37, 1, 3):                        # lengths with and without a vector tail
        w = scale_weights_rows(sig[:n], 0.1)
        for i in range(n):
            one = scale_weights(sig[i], 0.1)
            got = np.array([w.c_skip[i], w.c_out[i], w.c_in[i], w.c_noise[i]], dtype=np.float32)
            assert np.array_equal(got, np.array([one.c_skip, one.c_out, one.c_in, one.c_noise], dtype=np.float32)), (n, i)
    w = scale_weights_rows(torch.tensor([9.0, 1.0, 0.001]), 0.1)
    rows = np.stack([w.c_skip.numpy(), w.c_out.numpy(), w.c_in.numpy(), w.c_noise.numpy()], axis=1)
    assert np.array_equal(rows, g["scale_weights"])                          # the reference's values
    # loss_weight, diffusion.py:816-818, as train.py states it
    s = sig[:37]
    assert torch.equal(scale_weights_rows(s, 0.1).loss_weight, (s ** 2 + 0.1 ** 2) * (s * 0.1) ** -2)
    assert tuple(w.packed().shape) == (6, 3) and torch.equal(w.packed()[0], w.sigmas)


def test_class_surface_of_the_per_row_form():
    from moleculediffusiontransformer_amd import AnalogDiffusionFull, AnalogDiffusionSparse, KDiffusion_mod, UNetCFG1d
    for cls in (QMDiffusion, QMDiffusionForward, AnalogDiffusionSparse, AnalogDiffusionFull):
        p = inspect.signature(cls.eval_loss).parameters
        assert list(p)[:4] == ["self", "sequences", "output", "device"]
        for k in ("sigmas", "noise", "seed", "per_sample"):
            assert p[k].kind is inspect.Parameter.KEYWORD_ONLY
        assert p["per_sample"].default is False
    assert inspect.signature(KDiffusion_mod.denoise_fn).parameters["batched"].default is False
    assert inspect.signature(UNetCFG1d.forward).parameters["batched"].default is False
    for name in ("unet_eval_rows", "eval_loss", "precond_in_rows", "precond_out_rows"):
        assert hasattr(torch.ops.mdt, name)


def test_eval_loss_has_no_cpu_fallback():
    m = make_synth_model("tiny")
    g = load_golden("train_loss.npz")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.eval_loss(torch.from_numpy(g["seq"]), torch.from_numpy(g["x0"]), "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.unet(torch.from_numpy(g["x0"]), torch.from_numpy(g["sigmas"]), embedding=torch.zeros(3, 12, 128), batched=True)


def test_custom_ops_have_fake_registrations():
    """Shape inference of the per-row ops on meta tensors (no device, no engine)."""
    x = torch.empty(5, 16, 32, device="meta")
    pred = torch.empty(5, 32, 16, device="meta")
    v = torch.empty(5, device="meta")
    assert tuple(torch.ops.mdt.precond_in_rows(x, v, 16).shape) == (5, 32, 16)
    assert tuple(torch.ops.mdt.precond_out_rows(x, pred, v, v, 0.0).shape) == (5, 16, 32)
    assert tuple(torch.ops.mdt.unet_eval_rows(pred, torch.empty(5, 12, 128, device="meta"), v, 1.0, 0).shape) == (5, 32, 16)
    assert tuple(torch.ops.mdt.eval_loss(x, None, torch.empty(5, 12, 128, device="meta"), torch.empty(6, 5, device="meta"), 0, 0.0, 0,
                                         0).shape) == (5,)
