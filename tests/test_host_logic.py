"""CPU tests: host-side scalar logic, class surface, lowering (via the CPU program interpreter), C ABI export."""
import ctypes
import re
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
from helpers import CASES, oracle_cfg, synth_sd
from moleculediffusiontransformer_amd import (ADPM2Sampler, KarrasSchedule, QMDiffusion, QMDiffusionForward,
                                              runtime as rt)
from moleculediffusiontransformer_amd.compiler import compile_unet
from moleculediffusiontransformer_amd.diffusion import adpm2_plan, scale_weights
from moleculediffusiontransformer_amd.netspec import forward_unet_config, inverse_unet_config, sparse_unet_config
from oracle import unet_oracle as O
from oracle.program_interp import Buffers, run_program


def test_c_abi_exports_every_declared_symbol():
    lib = rt.load_library()
    hdr = open(os.path.join(ROOT, "include", "mdt_hip.h")).read()
    declared = set(re.findall(r"\b(mdt_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(rt.SYMBOLS)
    for name in declared:
        assert hasattr(lib, name)
    assert lib.mdt_abi_version() == rt.ABI_VERSION == 5      # (no MDT_ABI_TUNING_BIT: not a timing-only build)
    assert ctypes.sizeof(rt.MdtOp) == 8 + 10 * 16 + 24 * 4 + 8 * 4
    bad = rt.MdtOp()
    bad.kind = 1   # GEMM with cin == 0
    with pytest.raises(RuntimeError, match="cin must be"):
        rt.Program([bad])


def test_header_is_plain_c_and_the_binding_uses_its_numbers(tmp_path):
    """include/mdt_hip.h compiles as C99 on its own (it is what a cgo / JNI / ctypes binding reads), and every enumerator the Python
    binding mirrors (runtime.py: OP_*, G_*, N_*, F_*, ...) has the header's value."""
    import subprocess
    hdr = open(os.path.join(ROOT, "include", "mdt_hip.h")).read()
    names = sorted(set(re.findall(r"\b(MDT_[A-Z0-9]+_[A-Z0-9_]+) = -?\d", hdr)))        # enumerators are written "NAME = value"
    assert len(names) > 150
    src = tmp_path / "h.c"
    src.write_text('#include <stdio.h>\n#include "mdt_hip.h"\nint main(void) {\n' +
                   "".join(f'  printf("{n} %d\\n", (int){n});\n' for n in names) + "  return 0;\n}\n")
    exe = tmp_path / "h"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    values = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    checked = 0
    for n, v in values.items():
        py = n[4:]                                   # MDT_G_WFMT -> G_WFMT, MDT_OP_GEMM -> OP_GEMM
        if hasattr(rt, py) and isinstance(getattr(rt, py), int):
            assert getattr(rt, py) == int(v), (n, v, getattr(rt, py))
            checked += 1
    assert checked > 100


def test_plan_matches_reference_scalars():
    g = load_golden("scalars.npz")
    for T in (64, 100, 12):
        sig, steps = adpm2_plan(T, KarrasSchedule(0.001, 9.0, 3.0), ADPM2Sampler(rho=1), 0.1)
        assert np.array_equal(sig.numpy(), g[f"sigmas_{T}"])
        assert len(steps) == T - 1
        for i, s in enumerate(steps):
            assert np.float32(s.sigma_up) == np.float32(g[f"up_{T}"][i])
            assert np.float32(s.sigma_mid) == g[f"mid_{T}"][i]
            assert np.float32(s.dt_down) == np.float32(np.float32(g[f"down_{T}"][i]) - g[f"sigmas_{T}"][i])
            assert np.float32(s.dt_mid) == np.float32(g[f"mid_{T}"][i] - g[f"sigmas_{T}"][i])
    for row, s in zip(g["scale_weights"], (9.0, 1.0, 0.001)):
        w = scale_weights(torch.tensor(s), 0.1)
        assert np.array_equal(np.array([w.c_skip, w.c_out, w.c_in, w.c_noise], dtype=np.float32), row)
    # batch size does not change the to_batch()-ed scalars
    for s in (9.0, 0.37, 0.001):
        big = O.scale_weights(torch.full((1000,), s))
        w = scale_weights(torch.tensor(s), 0.1)
        assert float(big[0].flatten()[-1]) == w.c_skip and float(big[3][-1]) == w.c_noise


def test_class_surface_and_checkpoint_layout(capsys):
    g = load_golden("state_dict_keys.npz")
    m = QMDiffusion(max_length=64, pred_dim=16, channels=64, context_embedding_max_length=12,
                    text_embed_dim=64, embed_dim_position=64)
    assert "Using unet type:  cfg" in capsys.readouterr().out          # generative.py:740
    sd = m.state_dict()
    assert list(sd.keys()) == list(g["cfg1_keys"]) and len(sd) == 2301
    assert [v.numel() for v in sd.values()] == list(g["cfg1_numel"])
    assert sum(p.numel() for p in m.parameters()) == int(g["cfg1_nparams"]) == 32630960
    # the three aliases share storage
    assert sd["unet.to_mapping.0.weight"].data_ptr() == sd["diffusion.diffusion.net.to_mapping.0.weight"].data_ptr()
    for attr in ("unet", "diffusion", "fc1", "GELUact", "p_enc_1d", "max_length", "pred_dim", "unet_type"):
        assert hasattr(m, attr)
    assert m.diffusion.diffusion.alias == "k" and m.diffusion.net is m.unet
    # a checkpoint holding only unet.* restores the model under strict=False
    only_unet = {k: torch.zeros_like(v) for k, v in sd.items() if k.startswith("unet.")}
    m.load_state_dict(only_unet, strict=False)
    assert float(m.state_dict()["diffusion.net.to_mapping.0.weight"].abs().max()) == 0.0
    mf = QMDiffusionForward(64, 64, 1, None, 64, text_embed_dim=64, embed_dim_position=64)
    assert list(mf.state_dict().keys()) == list(g["cfg3_keys"])
    assert sum(p.numel() for p in mf.parameters()) == 18322684          # Forward_Diffusion.ipynb:1336
    big = QMDiffusion(max_length=32, pred_dim=22, channels=128, context_embedding_max_length=12,
                      text_embed_dim=64, embed_dim_position=64)
    assert sum(p.numel() for p in big.parameters()) == 90965554         # Inverse_Diffusion.ipynb:1580


def test_sparse_unet_keeps_the_reference_checkpoint_layout():
    """QMDiffusion(unet=UNetCFG1d(sparse_unet_config(...))): same state_dict keys and parameter count as the reference's
    AnalogDiffusionSparse(unet_type='cfg') (graphmodel.py:225-296), so its checkpoints load."""
    from moleculediffusiontransformer_amd.synth import make_synth_model
    g = load_golden("sparse_keys.npz")
    m = make_synth_model("sparse")
    assert list(m.state_dict().keys()) == list(g["keys"])
    assert sum(p.numel() for p in m.parameters()) == int(g["nparams"])


def test_analog_diffusion_wrappers_keep_the_reference_surface(capsys):
    """graphmodel.py:225-597: AnalogDiffusionSparse / AnalogDiffusionFull with the reference's constructor keywords, state_dict
    layout (Full: against the key list recorded from the reference) and pos_emb_fourier_add (text_embed_dim ==
    embed_dim_position); sample() refuses the CPU like the other classes."""
    from moleculediffusiontransformer_amd.graphmodel import AnalogDiffusionFull, AnalogDiffusionSparse
    from moleculediffusiontransformer_amd.synth import make_synth_model
    g = load_golden("full_keys.npz")
    m = make_synth_model("full")
    assert isinstance(m, AnalogDiffusionFull) and m.predict_neighbors is True and m.pos_emb_fourier_add is True
    assert list(m.state_dict().keys()) == list(g["keys"])
    assert sum(p.numel() for p in m.parameters()) == int(g["nparams"])
    assert m.unet.config.patch_size == 4 and m.unet.config.num_blocks == (3, 3) and m.unet.config.ctx_features == 64
    s = AnalogDiffusionSparse(max_length=128, channels=128, pred_dim=3, context_embedding_max_length=12, text_embed_dim=64,
                              embed_dim_position=64)
    assert "Using unet type" in capsys.readouterr().out
    gs = load_golden("sparse_keys.npz")
    assert list(s.state_dict().keys()) == list(gs["keys"]) and s.unet.config.patch_size == 8 and s.predict_neighbors is False
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s.sample(torch.zeros(2, 12), "cpu", cond_scale=1.0, timesteps=4)
    with pytest.raises(RuntimeError, match="text_embed_dim <= embed_dim_position"):     # x + p_enc_1d(x) does not broadcast there either
        AnalogDiffusionSparse(max_length=128, channels=128, pred_dim=3, pos_emb_fourier_add=True, text_embed_dim=128)
    # the additive conditioning prelude of the training path equals the oracle's
    from moleculediffusiontransformer_amd.train import conditioning_embedding
    seq = torch.from_numpy(load_golden("full_unet.npz")["seq"])
    emb = conditioning_embedding(m, seq)
    assert emb.shape == (2, 12, 64) and (emb - torch.from_numpy(load_golden("full_unet.npz")["emb"])).abs().max() < 1e-6


class _Rec(torch.nn.Module):
    def forward(self, output, embedding=None):
        self.output, self.embedding = output, embedding
        return torch.zeros(())


def test_analog_forward_slices_and_additive_prelude_match_the_reference():
    """ADVICE r3.  (i) AnalogDiffusionFull.forward is NOT the Sparse recipe (graphmodel.py:497-545: no padding, neighbour rows
    4 : 4 + max_length, the raw packed rows without predict_neighbors); Sparse pads xyz (+ max_neighbors rows) to max_length
    (:316-353) and, like the reference's pad_sequence, refuses sequences longer than max_length.  (ii) pos_emb_fourier_add with
    text_embed_dim < embed_dim_position adds the encoding's first text_embed_dim columns (transformer.py:3470).  Both against
    tensors recorded from the real reference (tests/golden/make_golden_r4.py)."""
    from moleculediffusiontransformer_amd.graphmodel import AnalogDiffusionFull, AnalogDiffusionSparse, pad_sequence
    g = load_golden("analog_forward.npz")
    seq, packed = torch.from_numpy(g["seq"]), torch.from_numpy(g["packed"])
    for pn in (False, True):
        sp = AnalogDiffusionSparse(max_length=16, channels=32, pred_dim=8 if pn else 3, context_embedding_max_length=12,
                                   text_embed_dim=64, embed_dim_position=64, predict_neighbors=pn)
        sp.diffusion = _Rec()
        sp.forward(seq, packed)
        assert torch.equal(sp.diffusion.output, torch.from_numpy(g[f"sparse_pn{int(pn)}_target"]))
        fu = AnalogDiffusionFull(max_length=16, channels=32, pred_dim=8, context_embedding_max_length=12, text_embed_dim=64,
                                 embed_dim_position=64, predict_neighbors=pn)
        fu.diffusion = _Rec()
        fu.forward(seq, packed)
        assert torch.equal(fu.diffusion.output, torch.from_numpy(g[f"full_pn{int(pn)}_target"]))
    with pytest.raises(RuntimeError, match="must match the existing size"):
        pad_sequence(torch.zeros(1, 3, 20), 16)
    a = load_golden("add_embed_d32.npz")
    m = AnalogDiffusionSparse(max_length=16, channels=32, pred_dim=3, context_embedding_max_length=12, pos_emb_fourier=True,
                              pos_emb_fourier_add=True, text_embed_dim=32, embed_dim_position=64)
    with torch.no_grad():
        m.fc1.weight.copy_(torch.from_numpy(a["fc1_w"]))
        m.fc1.bias.copy_(torch.from_numpy(a["fc1_b"]))
    m.diffusion = _Rec()
    m.forward(torch.from_numpy(a["seq"]), packed)
    assert m.diffusion.embedding.shape == (2, 12, 32) and m.unet.config.ctx_features == 32
    assert (m.diffusion.embedding - torch.from_numpy(a["emb"])).abs().max() < 1e-6


def test_no_cpu_fallback():
    m = QMDiffusion(max_length=32, pred_dim=16, channels=16, context_embedding_max_length=12,
                    text_embed_dim=64, embed_dim_position=64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.sample(torch.randn(2, 12), "cpu", cond_scale=1.0, timesteps=4)
    # the sampler seams need a HIP device too
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ADPM2Sampler(rho=1).step(torch.randn(2, 16, 32), lambda x, sigma: x, 1.0, 0.5)


def test_molecule_kernels_share_one_graph_row_header():
    """The graph row and the sets over it are defined once, in csrc/mdt_molrow.h: no header and no molecule kernel keeps a copy."""
    import glob
    csrc = os.path.join(ROOT, "moleculediffusiontransformer_amd", "csrc")
    files = sorted(glob.glob(os.path.join(csrc, "*.h")) + glob.glob(os.path.join(csrc, "k_mol*.hip")))
    assert os.path.join(csrc, "mdt_molrow.h") in files and len(files) > 20
    for path in files:
        text, name = open(path).read(), os.path.basename(path)
        for builtin in ("__builtin_popcountll", "__builtin_ctzll", "__builtin_clzll"):
            assert (builtin in text) == (name == "mdt_molrow.h"), (name, builtin)
        for helper in ("mol_popc", "mol_lowest", "mol_all", "mol_ring_adj"):
            defined = re.search(r"\b(?:int|void|bool|uint64_t)\s+" + helper + r"\s*\(", text) is not None
            assert defined == (name == "mdt_molrow.h"), (name, helper)
    assert "int mol_a(" not in open(os.path.join(csrc, "mdt_smiles_scan.h")).read()


def test_training_loss_matches_reference_formula():
    """QMDiffusion.forward (generative.py:812-833) -> KDiffusion_mod.forward (diffusion.py:820-844) as plain PyTorch with
    autograd (train.py): equal to the loss assembled from the pinned oracle's denoiser on the same sigmas / noise, and every
    parameter except the (unused at mask probability 0) FixedEmbedding receives a gradient, as in the reference."""
    from moleculediffusiontransformer_amd.synth import make_synth_model, synth_normal, synth_uniform
    from moleculediffusiontransformer_amd.train import conditioning_embedding, kdiffusion_loss
    for case in ("tiny", "cfg3"):
        kind, kw = CASES[case]
        m = make_synth_model(case)
        sd, cfg = synth_sd(case), oracle_cfg(case)
        B = 3
        seq = synth_normal(f"train/{case}/seq", (B, kw["context_embedding_max_length"]))
        x0 = synth_normal(f"train/{case}/x0", (B, kw["pred_dim"], kw["max_length"])).clamp(-1, 1) * 0.5
        noise = synth_normal(f"train/{case}/noise", tuple(x0.shape))
        sigmas = (-1.2 + 1.2 * synth_normal(f"train/{case}/sig", (B,))).exp()
        emb = conditioning_embedding(m, seq)
        assert (emb - O.cond_embed(sd, cfg, seq)).abs().max() < 1e-6
        loss = kdiffusion_loss(m, x0, noise, emb, sigmas=sigmas)
        with torch.no_grad():
            xn = x0 + sigmas.view(-1, 1, 1) * noise
            den = torch.cat([O.denoise(sd, cfg, xn[b:b + 1], sigmas[b], O.cond_embed(sd, cfg, seq[b:b + 1])) for b in range(B)])
            per = ((den - x0) ** 2).flatten(1).mean(1) * ((sigmas ** 2 + 0.01) * (sigmas * 0.1) ** -2)
        assert abs(float(loss.detach()) - float(per.mean())) < 1e-4 * max(1.0, float(per.mean()))
        loss.backward()
        missing = [n for n, p_ in m.named_parameters() if p_.grad is None]
        assert missing == ["unet.fixed_embedding.embedding.weight"]
        assert all(torch.isfinite(p_.grad).all() for p_ in m.parameters() if p_.grad is not None)
    # the public call: random sigmas / noise from the global generator, reproducible under a seed
    torch.manual_seed(3)
    a = m(seq, x0)
    torch.manual_seed(3)
    b = m(seq, x0)
    assert a.requires_grad and torch.equal(a.detach(), b.detach())


def test_training_loss_honours_dynamic_threshold_like_the_reference():
    """the training objective goes through denoise_fn, whose clip() reads KDiffusion_mod.dynamic_threshold
    (diffusion.py:814, :75-88).  QMDiffusion.forward of the tiny model against the loss the REAL reference returned on the same
    sigmas / noise with the threshold at 0.0 and 0.9 (tests/golden/make_golden_r4.py train_loss); the analog wrappers' recorded
    conditioning embeddings (now from synthetic fc1 weights: reproducible) ride along."""
    from moleculediffusiontransformer_amd.synth import make_synth_model
    from moleculediffusiontransformer_amd.train import conditioning_embedding, kdiffusion_loss
    g = load_golden("train_loss.npz")
    m = make_synth_model("tiny")
    seq, x0 = torch.from_numpy(g["seq"]), torch.from_numpy(g["x0"])
    noise, sigmas = torch.from_numpy(g["noise"]), torch.from_numpy(g["sigmas"])
    emb = conditioning_embedding(m, seq)
    got = {}
    for q in (0.0, 0.9):
        m.diffusion.diffusion.dynamic_threshold = q
        got[q] = float(kdiffusion_loss(m, x0, noise, emb, sigmas=sigmas).detach())
        ref = float(g[f"loss_q{q}"])
        assert abs(got[q] - ref) < 2e-5 * abs(ref), (q, got[q], ref)
    assert abs(got[0.9] - got[0.0]) > 1.0              # the fixture really exercises the quantile branch
    from moleculediffusiontransformer_amd.graphmodel import AnalogDiffusionSparse
    from moleculediffusiontransformer_amd.synth import synth_normal
    a = load_golden("analog_forward.npz")
    for pn in (False, True):
        sp = AnalogDiffusionSparse(max_length=16, channels=32, pred_dim=8 if pn else 3, context_embedding_max_length=12,
                                   text_embed_dim=64, embed_dim_position=64, predict_neighbors=pn)
        with torch.no_grad():
            sp.fc1.weight.copy_(synth_normal("r4/analog/fc1_w", tuple(sp.fc1.weight.shape)))
            sp.fc1.bias.copy_(synth_normal("r4/analog/fc1_b", tuple(sp.fc1.bias.shape)))
        sp.diffusion = _Rec()
        sp.forward(torch.from_numpy(a["seq"]), torch.from_numpy(a["packed"]))
        assert (sp.diffusion.embedding - torch.from_numpy(a[f"sparse_pn{int(pn)}_emb"])).abs().max() < 1e-6


def test_sampler_seams_exist_with_reference_signatures():
    """diffusion.py:347-366 (Sampler), :486-549 (ADPM2Sampler), :554-591 (DiffusionSampler), :594-625 (DiffusionInpainter),
    :724-767 (XDiffusion_x.sample / inpaint): the mix-and-match seams of SURVEY section 8(b)."""
    import inspect
    from moleculediffusiontransformer_amd import DiffusionInpainter, DiffusionSampler, Sampler
    s = ADPM2Sampler(rho=1)
    assert isinstance(s, Sampler) and "k" in [t.alias for t in s.diffusion_types]
    assert list(inspect.signature(s.forward).parameters) == ["noise", "fn", "sigmas", "num_steps"]
    assert list(inspect.signature(s.step).parameters)[:4] == ["x", "fn", "sigma", "sigma_next"]
    assert list(inspect.signature(s.inpaint).parameters) == ["source", "mask", "fn", "sigmas", "num_steps", "num_resamples"]
    m = QMDiffusion(max_length=32, pred_dim=16, channels=16, context_embedding_max_length=12, text_embed_dim=64,
                    embed_dim_position=64)
    ds = DiffusionSampler(m.diffusion.diffusion, sampler=s, sigma_schedule=KarrasSchedule(0.001, 9.0, 3.0), num_steps=4,
                          clamp=False)
    assert ds.denoise_fn == m.diffusion.diffusion.denoise_fn
    DiffusionInpainter(m.diffusion.diffusion, num_steps=4, num_resamples=1, sampler=s,
                       sigma_schedule=KarrasSchedule(0.001, 9.0, 3.0))

    class Other:
        alias = "v"
        denoise_fn = None
    with pytest.raises(AssertionError, match="incompatible"):
        DiffusionSampler(Other(), sampler=s, sigma_schedule=KarrasSchedule(0.001, 9.0, 3.0))
    with pytest.raises(AssertionError, match="sigma"):
        m.diffusion.diffusion.denoise_fn(torch.zeros(1, 16, 32), embedding=torch.zeros(1, 12, 128))


def test_token_chain_between_the_two_models():
    """reverse_tokenize -> texts_to_sequences -> pad_sequences(post, post) -> / X_norm_factor (generative.py:1069-1078,
    :425-429) restated on ids: zeros dropped, order kept, padded / truncated at the end."""
    from moleculediffusiontransformer_amd import tokens_to_forward_input
    t = torch.tensor([[3, 0, 5, 0, 1, 7], [0, 0, 0, 2, 2, 0], [0, 0, 0, 0, 0, 0]])
    out = tokens_to_forward_input(t, 8, 2.0)
    assert out.tolist() == [[1.5, 2.5, 0.5, 3.5, 0, 0, 0, 0], [1.0, 1.0, 0, 0, 0, 0, 0, 0], [0.0] * 8]
    assert tokens_to_forward_input(t, 3).tolist() == [[3.0, 5.0, 1.0], [2.0, 2.0, 0.0], [0.0, 0.0, 0.0]]


@pytest.mark.parametrize("mode", ["f32", "f32-wide", "f32-layers", "bf16x3", "bf16x3-wide", "bf16"])
@pytest.mark.parametrize("case", ["tiny", "pd22", "cfg3", "cfg1", "sparse", "full"])
def test_lowering_matches_reference_golden(case, mode, monkeypatch):
    """compiler.py's op program, executed by the CPU interpreter, reproduces the reference U-Net output ('bf16': the
    reduced-precision mode, within its own budget of 2e-2 of an O(1) output per evaluation).  'f32' is the exact-fp32 mode on
    the SAME fused program as the default mode (fp32 fragment tiles in the ring kernels' ops), 'f32-layers' its layer-by-layer
    form (MDT_F32_FUSED=0)."""
    if mode == "f32-layers":
        monkeypatch.setenv("MDT_F32_FUSED", "0")
    kind, kw = CASES[case]
    if kind == "full":
        ucfg = sparse_unet_config(kw["pred_dim"], kw["channels"], 64, kw["context_embedding_max_length"], patch_size=4, num_blocks=(3, 3))
    else:
        mk = {"inverse": inverse_unet_config, "forward": forward_unet_config, "sparse": sparse_unet_config}[kind]
        ucfg = mk(kw["pred_dim"], kw["channels"], 128, kw["context_embedding_max_length"])
    usd = {k[5:]: v for k, v in synth_sd(case).items() if k.startswith("unet.")}
    wide = mode.endswith("-wide")       # 256-channel transformers as whole-transformer launches (k_tf256)
    layers = mode.endswith("-layers")
    mode = mode.split("-")[0]
    if wide and case not in ("cfg1", "sparse"):
        pytest.skip("no 256-channel fused transformer in this configuration")
    cu = compile_unet(ucfg, kw["max_length"], kw["context_embedding_max_length"], usd, max_time_rows=4,
                      gemm_mode=mode, tf256=wide)
    if wide:
        assert any(op.kind == rt.OP_TF256 for op in cu.programs["eval"])
    ring = (rt.OP_TF128, rt.OP_TF256, rt.OP_RCONV, rt.OP_RESBLOCK, rt.OP_TBLOCK)
    if mode == "f32" and layers:
        assert not any(op.kind in ring for op in cu.programs["eval"])
    elif mode == "f32" and case == "cfg1":
        # the fused program of the default mode, op for op, with fp32 fragment tiles
        ref = compile_unet(ucfg, kw["max_length"], kw["context_embedding_max_length"], usd, max_time_rows=4, gemm_mode="bf16x3", tf256=wide)
        assert [op.kind for op in cu.programs["eval"]] == [op.kind for op in ref.programs["eval"]] and len(cu.programs["eval"]) == 20
        wf = {rt.OP_TF128: rt.F_WF32, rt.OP_TF256: rt.F_WF32, rt.OP_RCONV: rt.R_WF32, rt.OP_RESBLOCK: rt.K_WF32}
        assert all(op.i[wf[op.kind]] == 1 for op in cu.programs["eval"] if op.kind in wf)
        assert all(op.i[wf[op.kind]] == 0 for op in ref.programs["eval"] if op.kind in wf)
        assert all(op.a2.space == rt.SP_NONE for op in cu.programs["eval"] if op.kind == rt.OP_GEMM)     # exact fp32 GEMMs: no lo plane
    if mode == "bf16" and case in ("cfg1", "cfg3", "sparse"):
        assert any(op.kind == rt.OP_PREP16 for op in cu.programs["eval"])       # regular layers: bf16 x bf16 GEMM
        assert any(op.kind == rt.OP_GEMM and op.i[rt.G_WFMT] == 6 for op in cu.programs["eval"])   # bf16 hidden layer
    tol = 1e-5 if mode == "f32" else 5e-5      # split weights carry ~2^-17 relative rounding
    if mode == "bf16":
        tol = 2e-2
    g = load_golden(f"{case}_unet.npz")
    x, t, emb = (torch.from_numpy(g[k]) for k in ("x", "t", "emb"))
    B, C, L = x.shape
    for fixed in (False, True):
        outs = []
        for b in range(min(B, 2) if fixed else B):
            act, shr = torch.zeros(cu.act_floats), torch.zeros(cu.shr_floats)
            xin = torch.zeros(1, L, cu.in_pad)
            xin[0, :, :C] = x[b].T
            out = torch.zeros(1, L, cu.in_pad)
            bufs = Buffers(cu.weights, act, shr, {0: xin.view(-1), 1: emb[b:b + 1].contiguous().view(-1), 2: out.view(-1)})
            shr[cu.shr["c_noise"]] = t[b]
            run_program(cu.programs["time"], bufs, 1, 1)
            ss = cu.ss_total
            shr[cu.shr["ss_cur"]: cu.shr["ss_cur"] + ss] = shr[cu.shr["ss_all"]: cu.shr["ss_all"] + ss].clone()
            run_program(cu.programs["ctx_fixed" if fixed else "ctx"], bufs, 1)
            run_program(cu.programs["eval_fixed" if fixed else "eval"], bufs, 1)
            outs.append(out[0, :, :C].T.clone())
            assert float(out[0, :, C:].abs().max()) == 0.0 if cu.in_pad > C else True
        y = torch.stack(outs)
        if not fixed:
            assert (y - torch.from_numpy(g["y_scale1"])).abs().max() < tol
            y_cond = y
        else:
            mix = y + (y_cond[: y.shape[0]] - y) * 7.5
            assert (mix - torch.from_numpy(g["y_scale7p5"])[: y.shape[0]]).abs().max() < (10 * tol if mode != "bf16" else 0.3)
    assert abs(cu.flops_per_sample_eval - {"cfg1": 388.7e6}.get(case, cu.flops_per_sample_eval)) < 1e6


_RING_UNITS = ("k_tblock32", "k_rconv", "k_tf128", "k_tf256", "k_rconv_f32", "k_tf128_f32", "k_tf256_f32", "k_attn", "k_res256", "k_proj")


@pytest.fixture(scope="module")
def ring_kernel_reports():
    """One device-only hipcc run per ring-kernel translation unit (build.py's flags): resource remarks + the assembly for the ISA lint."""
    import shutil
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    import isa_lint
    import kernel_resources
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=4) as ex:          # (one device-only compile per unit serves both)
        both = list(ex.map(kernel_resources.resources_and_assembly, _RING_UNITS))
    res = [b[0] for b in both]
    lint = [isa_lint.lint_unit(u, asm=b[1]) for u, b in zip(_RING_UNITS, both)]
    return dict(zip(_RING_UNITS, res)), dict(zip(_RING_UNITS, lint))


def test_ring_kernels_keep_their_arrays_in_registers(ring_kernel_reports):
    """A register array that hipcc decides to index dynamically moves to scratch; in a loader wave every scratch load is
    then waited for with vmcnt(0) and the whole LDS-DMA stream serialises (seen twice: 2-5x slower kernels, all tests
    green), and a spill next to an in-flight inline-asm ds_read stores a register that has not landed yet.  Compile the ring
    kernels with resource remarks and bound their scratch use.  Round 4: ZERO for k_tf128 (all instantiations), for the
    k_rconv forms on the default path, for every exact-fp32 instantiation (*_f32 units) and for k_tf256 except the pair-split
    cross-attention instantiations, which keep 12 bytes (threadIdx.x and the lane group, stored once after to_in and reloaded
    once behind the block loop; 120 when round 3 ended, 228 when round 2 ended).  How k_tf256 got there: addresses and masks
    that are needed once per sub-block or head are formed WHERE THEY ARE USED from an opaque lane id (k_tf256.hip: lane_now,
    cross_consts, self_mask) instead of living for the whole launch, and the exact-fp32 phase keeps two sets of one fragment
    pair (16 registers) instead of three full sets (48)."""
    import re
    res, _ = ring_kernel_reports
    # The exact-fp32 instantiations (round 4: *_f32 units) are all at ZERO: k_tf256's fp32 phase needs two fragment sets instead
    # of three (a unit is 512 MFMA-pipe cycles, one unit of read-ahead covers the LDS latency), which is what the split form lacks.
    limits = {"k_tblock32": 24, "k_rconv": 0, "k_tf128": 0, "k_tf256": 16,      # bytes per lane
              "k_rconv_f32": 0, "k_tf128_f32": 0, "k_tf256_f32": 0,
              "k_attn": 0,        # k_attn_ctx (round 4: context streamed through a per-wave LDS ring, inline-asm fragment reads)
              "k_res256": 0,      # round 5: the chained ResNet blocks of the 256-channel level (all 8 instantiations)
              "k_proj": 0}        # round 5: the row-stationary projection on ring tiles (all 12 instantiations)
    for name, limit in limits.items():
        assert res[name], name
        for fn, v in res[name]:
            if name == "k_attn" and "k_attn_ctx" not in fn:
                continue
            if name.startswith("k_rconv") and re.search(r"ELi2ELi[01]ELb[01]EEEvNS_9RConvArgsE$", fn):
                # two-source instantiations <..., NSRC = 2, PRO, F32>: only the 1x1 form without a prologue (PRO = 0) is on the
                # default path (the concatenated inputs' residual convolution; C = 128, or C = 256 with the output channels
                # split over two workgroups)
                if not re.search(r"(ELi4ELi128ELi1ELi1ELi2ELi0|ELi2ELi256ELi1ELi2ELi2ELi0)ELb[01]EEEvNS_9RConvArgsE$", fn):
                    continue
            assert 0 <= v["scratch"] <= limit, (fn, v)
            if name == "k_tf256" and not re.search(r"ILi[1-6]ELi2ELb0E", fn):      # everything but <NPW >= 1, NSPLIT = 2, split-bf16>
                assert v["scratch"] == 0, (fn, v)


def test_no_instruction_touches_an_in_flight_fragment_read(ring_kernel_reports):
    """tools/isa_lint.py on the compiler's assembly of every ring kernel: inside every basic block, no instruction reads or
    writes the destination registers of a ds_read before an s_waitcnt lgkmcnt that covers it (hipcc treats the inline-asm
    fragment reads as complete where they are issued, so a copy / spill / re-use placed right behind one would move a
    register that has not landed)."""
    import isa_lint
    # the lint itself: a copy right behind a read is caught, the same copy behind a covering wait is not, and a counted wait
    # retires exactly the reads with enough younger LDS operations
    rd = "ds_read_b128 v[4:7], v1 offset:0"
    assert len(isa_lint.lint_kernel([rd, "v_mov_b32_e32 v8, v5", "s_waitcnt lgkmcnt(0)"])) == 1
    assert isa_lint.lint_kernel([rd, "s_waitcnt lgkmcnt(0)", "v_mov_b32_e32 v8, v5"]) == []
    two = [rd, "ds_read_b128 v[8:11], v1 offset:256", "s_waitcnt lgkmcnt(1)"]
    assert isa_lint.lint_kernel(two + ["v_mfma_f32_16x16x32_bf16 v[20:23], v[4:7], v[12:15], v[20:23]"]) == []
    assert len(isa_lint.lint_kernel(two + ["v_mfma_f32_16x16x32_bf16 v[20:23], v[8:11], v[12:15], v[20:23]"])) == 1
    assert len(isa_lint.lint_kernel([rd, "scratch_store_dword off, v6, off offset:4", "s_waitcnt lgkmcnt(0)"])) == 1
    # round 4: the same for vector-memory loads (vmcnt counts loads, stores and LDS-DMA of the wave, in issue order)
    gl = "global_load_dword v9, v[2:3], off"
    assert len(isa_lint.lint_kernel([gl, "v_or_b32_e32 v10, v10, v9", "s_waitcnt vmcnt(0)"])) == 1
    assert isa_lint.lint_kernel([gl, "s_waitcnt vmcnt(0)", "v_or_b32_e32 v10, v10, v9"]) == []
    dma = "global_load_lds_dwordx4 v[4:5], off"                 # LDS-DMA: counts in vmcnt, no landing register
    assert isa_lint.lint_kernel([gl, dma, "s_waitcnt vmcnt(1)", "v_mov_b32_e32 v11, v9"]) == []
    assert len(isa_lint.lint_kernel([gl, dma, "s_waitcnt vmcnt(2)", "v_mov_b32_e32 v11, v9"])) == 1
    assert len(isa_lint.lint_kernel(["buffer_load_dwordx4 v[20:23], v1, s[4:7], 0 offen sc1", "v_add_f32_e32 v30, v21, v30"])) == 1
    assert isa_lint.lint_kernel([gl, "global_load_dword v9, v[2:3], off offset:128", "s_waitcnt vmcnt(0)", "v_mov_b32_e32 v1, v9"]) == []
    _, lint = ring_kernel_reports
    for name, (report, n_reads) in lint.items():
        assert n_reads > (50 if name == "k_attn" else 100), (name, n_reads)
        for kernel, violations in report.items():
            assert not violations, (name, kernel, violations[:3])


@pytest.mark.parametrize("mode", ["bf16x3", "f32"])
@pytest.mark.parametrize("cin,cout", [(16, 64), (64, 16)])
def test_fused_resnet_block_lowering(cin, cout, mode):
    """MDT_OP_RESBLOCK on the CPU side: the compiler's MFMA-fragment packing (k-steps enumerate (tap, channel) pairs,
    lane i + 16 g holds pairs 8 g .. 8 g + 7 of weight row i) and the interpreter's unpacking are inverse to each other,
    and the interpreted op is the reference ResnetBlock1d (modules.py:145-205) with one GroupNorm group."""
    from moleculediffusiontransformer_amd import runtime as rt
    from moleculediffusiontransformer_amd.compiler import Ten, UNetCompiler
    g = torch.Generator().manual_seed(7)
    r = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale   # noqa: E731
    p = "blk."
    sd = {p + "block1.groupnorm.weight": 1 + 0.1 * r(cin), p + "block1.groupnorm.bias": 0.1 * r(cin),
          p + "block1.project.weight": r(cout, cin, 3, scale=(3 * cin) ** -0.5), p + "block1.project.bias": 0.1 * r(cout),
          p + "block2.groupnorm.weight": 1 + 0.1 * r(cout), p + "block2.groupnorm.bias": 0.1 * r(cout),
          p + "block2.project.weight": r(cout, cout, 3, scale=(3 * cout) ** -0.5), p + "block2.project.bias": 0.1 * r(cout),
          p + "to_out.weight": r(cout, cin, 1, scale=cin ** -0.5), p + "to_out.bias": 0.1 * r(cout)}
    comp = UNetCompiler(inverse_unet_config(16, 64, 128, 12), 64, 12, sd, gemm_mode=mode)
    comp.resnet(Ten(rt.SP_ACT, 0, 64, cin), p, cin, cout, 1, free_input=False)
    assert [op.kind for op in comp.ops] == [rt.OP_RESBLOCK]
    op = comp.ops[0]
    assert op.i[rt.K_WF32] == int(mode == "f32")
    op.out = rt.MdtRef(rt.SP_ACT, 0, 64 * cin)
    op.p3 = rt.MdtRef(rt.SP_SHR, 0, 0)
    B = 3
    shr = 0.3 * r(2 * cout)
    x = r(B, 64, cin) * 1.5 + 0.3
    bufs = Buffers(comp.W.pack(), torch.cat([x.reshape(-1), torch.zeros(B * 64 * cout)]), shr, {})
    run_program([op], bufs, B, 0)
    F = torch.nn.functional
    xt = x.transpose(1, 2)
    h = F.conv1d(F.silu(F.group_norm(xt, 1, sd[p + "block1.groupnorm.weight"], sd[p + "block1.groupnorm.bias"], 1e-5)),
                 sd[p + "block1.project.weight"], sd[p + "block1.project.bias"], padding=1)
    h = F.group_norm(h, 1, sd[p + "block2.groupnorm.weight"], sd[p + "block2.groupnorm.bias"], 1e-5)
    h = h * (shr[:cout].view(1, cout, 1) + 1) + shr[cout:].view(1, cout, 1)
    y = F.conv1d(F.silu(h), sd[p + "block2.project.weight"], sd[p + "block2.project.bias"], padding=1)
    y = (y + F.conv1d(xt, sd[p + "to_out.weight"], sd[p + "to_out.bias"])).transpose(1, 2)
    got = bufs.act[B * 64 * cin:].view(B, 64, cout)
    assert (got - y).abs().max() < 1e-4        # weights pass through bf16 hi + lo (2^-17 relative)


def test_bench_power_sampler_is_optional():
    """bench.py's socket-power sampler reads amdgpu hwmon files of the rank's GPU; without them (this CPU container, or a
    box that hides sysfs) it must yield None instead of failing the bench line."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    s = mod.PowerSampler(0)
    assert s.dir is None
    s.start()
    s.join(timeout=2)
    assert s.summary() is None


def test_bench_dump_outputs_stays_within_its_budget(tmp_path, monkeypatch):
    """bench.py --dump-outputs: a tensor within the budget is written whole as float32; a larger one as a fixed sample of its
    rows, in row order, the same in every run."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    x = torch.randn(40, 4, 8)
    mod.dump_outputs(x, str(tmp_path / "whole"))
    got = np.load(tmp_path / "whole" / "samples.npy")
    assert got.dtype == np.float32 and np.array_equal(got, x.numpy())
    monkeypatch.setattr(mod, "DUMP_LIMIT_BYTES", 10 * 4 * 8 * 4 + 100)       # room for 10 rows
    mod.dump_outputs(x, str(tmp_path / "a"))
    mod.dump_outputs(x.clone(), str(tmp_path / "b"))
    a, b = np.load(tmp_path / "a" / "samples.npy"), np.load(tmp_path / "b" / "samples.npy")
    assert a.shape == (10, 4, 8) and a.dtype == np.float32 and np.array_equal(a, b)
    rows = [int(np.flatnonzero((x.numpy() == r).all(axis=(1, 2)))[0]) for r in a]
    assert rows == sorted(rows) and len(set(rows)) == 10


def test_torch_library_ops_are_registered_and_refuse_cpu_tensors():
    """SURVEY section 8(b), last row: the native boundary as a torch.library namespace.  Every op of torch.ops.mdt has a
    schema and shape inference (meta tensors, no GPU needed) and raises RuntimeError for non-HIP tensors (TORCH_CHECK
    convention; there is no CPU implementation behind the ops)."""
    import moleculediffusiontransformer_amd.ops as ops  # noqa: F401  (registers the namespace)
    names = ["cond_embed", "precond_in", "precond_out", "cfg_mix", "adpm2_mid", "adpm2_next", "adpm2_euler", "argmax_tokens",
             "unet_eval", "sample", "all_gather_samples"]
    for n in names:
        assert hasattr(torch.ops.mdt, n), n
    m = lambda *s, dt=torch.float32: torch.empty(*s, device="meta", dtype=dt)   # noqa: E731
    assert torch.ops.mdt.cond_embed(m(3, 12), m(64, 1), m(64), m(32), 64).shape == (3, 12, 128)
    assert torch.ops.mdt.precond_in(m(3, 16, 64), 0.5, 16).shape == (3, 64, 16)
    assert torch.ops.mdt.precond_out(m(3, 16, 64), m(3, 64, 16), 0.1, 0.2).shape == (3, 16, 64)
    xm, xin = torch.ops.mdt.adpm2_mid(m(3, 22, 32), m(3, 32, 32), 0.1, 0.2, 1.0, -0.1, 0.3)
    assert xm.shape == (3, 22, 32) and xin.shape == (3, 32, 32)
    assert torch.ops.mdt.argmax_tokens(m(3, 16, 64)).dtype == torch.int32
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        torch.ops.mdt.cond_embed(torch.zeros(3, 12), torch.zeros(64, 1), torch.zeros(64), torch.zeros(32), 64)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        torch.ops.mdt.precond_in(torch.zeros(3, 16, 64), 0.5, 16)
    with pytest.raises(RuntimeError):
        torch.ops.mdt.unet_eval(torch.zeros(1, 64, 16), torch.zeros(1, 12, 128), 0.0, 1.0, 987654)


# Every compile-time switch of compiler.py / DESIGN.md 10 that turns a fused form back into its previous form: (variable, value, cases).
# "a switch that no test flips is a dead configuration" -- each is flipped here (lowering against the reference's golden
# U-Net output through the CPU interpreter) and on the GPU (tests/test_gpu_parity.py::test_every_fallback_switch_matches_reference).
FALLBACK_SWITCHES = [
    ("MDT_TF128", "0", ("cfg1",)), ("MDT_RES128", "0", ("cfg1",)), ("MDT_TF256_PAIR", "0", ("cfg1",)), ("MDT_PAIR_STRIDE", "1", ("cfg1",)),
    ("MDT_RCONV", "0", ("cfg1",)), ("MDT_RCONV2", "1", ("cfg1+MDT_RES256=0",)), ("MDT_RCONV2", "0", ("cfg1+MDT_RES256=0",)),
    ("MDT_RESBLOCK", "0", ("cfg1", "cfg3")),
    ("MDT_RES256", "1", ("cfg1",)), ("MDT_RES256", "0", ("cfg3",)), ("MDT_RES256", "whole", ("cfg1",)), ("MDT_PROJ", "0", ("cfg1", "cfg3")), ("MDT_FOLD_PATCH", "0", ("cfg3", "full")),
    ("MDT_PATCH_CONV", "0", ("cfg1", "cfg3")), ("MDT_FOLD_CTX", "0", ("cfg3",)), ("MDT_T1_FOLD", "0", ("cfg3",)), ("MDT_CTX_SPLIT", "0", ("cfg3",)),
    ("MDT_FOLD_OUT", "0", ("cfg1",)), ("MDT_QKV_MERGE", "0", ("cfg3",)), ("MDT_B16", "0", ("cfg1",)), ("MDT_CFG_DUAL", "0", ("cfg1",)),
    ("MDT_RES16", "0", ("cfg1",)), ("MDT_LNFOLD", "0", ("cfg1",)), ("MDT_CAT_FOLD", "0", ("cfg1",)),
]


def _lowered_eval(case, mode, extra_env, monkeypatch, rows=(0,), wide=False):
    for k, v in extra_env.items():
        monkeypatch.setenv(k, v)
    kind, kw = CASES[case]
    if kind == "full":
        ucfg = sparse_unet_config(kw["pred_dim"], kw["channels"], 64, kw["context_embedding_max_length"], patch_size=4, num_blocks=(3, 3))
    else:
        mk = {"inverse": inverse_unet_config, "forward": forward_unet_config, "sparse": sparse_unet_config}[kind]
        ucfg = mk(kw["pred_dim"], kw["channels"], 128, kw["context_embedding_max_length"])
    usd = {k[5:]: v for k, v in synth_sd(case).items() if k.startswith("unet.")}
    cu = compile_unet(ucfg, kw["max_length"], kw["context_embedding_max_length"], usd, max_time_rows=4, gemm_mode=mode, tf256=wide)
    g = load_golden(f"{case}_unet.npz")
    x, t, emb = (torch.from_numpy(g[k]) for k in ("x", "t", "emb"))
    _, C, L = x.shape
    outs = []
    for b in rows:
        act, shr = torch.zeros(cu.act_floats), torch.zeros(cu.shr_floats)
        xin = torch.zeros(1, L, cu.in_pad)
        xin[0, :, :C] = x[b].T
        out = torch.zeros(1, L, cu.in_pad)
        bufs = Buffers(cu.weights, act, shr, {0: xin.view(-1), 1: emb[b:b + 1].contiguous().view(-1), 2: out.view(-1)})
        shr[cu.shr["c_noise"]] = t[b]
        run_program(cu.programs["time"], bufs, 1, 1)
        ss = cu.ss_total
        shr[cu.shr["ss_cur"]: cu.shr["ss_cur"] + ss] = shr[cu.shr["ss_all"]: cu.shr["ss_all"] + ss].clone()
        run_program(cu.programs["ctx"], bufs, 1)
        run_program(cu.programs["eval"], bufs, 1)
        outs.append(out[0, :, :C].T.clone())
    return cu, (torch.stack(outs) if outs else None), torch.from_numpy(g["y_scale1"])[list(rows)]


@pytest.mark.parametrize("var,value,cases", FALLBACK_SWITCHES, ids=[f"{v}={x}" for v, x, _ in FALLBACK_SWITCHES])
def test_every_fallback_switch_lowers_to_the_reference_result(var, value, cases, monkeypatch):
    """Each switch changes the op program (or is recorded as having no effect on that configuration) and the changed program
    still reproduces the reference's U-Net output."""
    changed = False
    for case in cases:
        mode = "bf16" if var in ("MDT_B16", "MDT_QKV_MERGE", "MDT_RES16", "MDT_LNFOLD", "MDT_CAT_FOLD") else "bf16x3"   # the switches of the reduced-precision mode
        # "case+VAR=v": the switch acts on a form that is itself a fallback since round 6 (the two-source k_rconv launches of the up
        # path: the chains took them over) -- flipped on top of that fallback
        case, _, under = case.partition("+")
        env0 = dict([under.split("=")]) if under else {}
        base, _, _ = _lowered_eval(case, mode, env0, monkeypatch, rows=())
        cu, y, ref = _lowered_eval(case, mode, {**env0, var: value}, monkeypatch)
        sig = lambda c: [(op.kind, tuple(op.i)) for name in ("eval", "ctx") for op in c.programs[name]] + \
            [len(c.programs.get("eval_dual", []))]                                # noqa: E731
        changed |= sig(base) != sig(cu)
        assert (y - ref).abs().max() < (2e-2 if mode == "bf16" else 5e-5), (var, value, case)
        monkeypatch.delenv(var)
        for k_ in env0:
            monkeypatch.delenv(k_)
    assert changed, f"{var}={value} changes nothing in {cases}: a dead switch"
