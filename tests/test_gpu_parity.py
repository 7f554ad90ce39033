"""-m gpu: the HIP sampling path against golden vectors from the real reference and against the oracle.

Tolerance: the north star asks for <= 1e-4 max-abs deviation from the fp32 CPU reference on identical
noise; the tests assert 1e-4 on final samples and intermediate sampler states, 5e-5 on single evaluations.
"""
import pytest
import torch

from conftest import load_golden
from gpu_util import DEV, make_model
from helpers import noise_fns, oracle_cfg, synth_sd, to_t
from moleculediffusiontransformer_amd import NoiseSource
from moleculediffusiontransformer_amd.synth import synth_normal
from oracle import unet_oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-4


@pytest.fixture(scope="module", params=["bf16x3", "f32", "f32-layers"])
def models(request):
    """Every parity test runs with both product types on the SAME fused program -- split-bf16 MFMA (default) and exact fp32
    MFMA ('f32': fp32 fragment tiles in the ring kernels) -- and with the exact mode's layer-by-layer form (MDT_F32_FUSED=0:
    k_gemm + k_attn + k_gn_act, the second exact implementation)."""
    import os
    cache = {}
    mode, _, form = request.param.partition("-")
    old = os.environ.get("MDT_F32_FUSED")
    os.environ["MDT_F32_FUSED"] = "0" if form == "layers" else "1"      # read when an engine is compiled

    def get(case):
        if case not in cache:
            cache[case] = make_model(case)
            cache[case].gemm_mode = mode
        return cache[case]
    get.mode = mode
    yield get
    if old is None:
        del os.environ["MDT_F32_FUSED"]
    else:
        os.environ["MDT_F32_FUSED"] = old


@pytest.mark.parametrize("case", ["tiny", "pd22", "cfg3", "cfg1", "nb", "sparse", "full"])
def test_unet_eval_and_denoise_match_reference(models, case):
    g = load_golden(f"{case}_unet.npz")
    m = models(case)
    emb = m._embed(to_t(g["seq"]), DEV)
    assert (emb.cpu() - to_t(g["emb"])).abs().max() < 1e-6
    x, t = to_t(g["x"]).to(DEV), to_t(g["t"])
    for b in range(x.shape[0]):            # the golden batch uses a different time per row
        y = m.unet(x[b:b + 1], t[b:b + 1], embedding=emb[b:b + 1], embedding_scale=1.0)
        assert (y.cpu() - to_t(g["y_scale1"])[b:b + 1]).abs().max() < 5e-5, (case, b)
        y = m.unet(x[b:b + 1], t[b:b + 1], embedding=emb[b:b + 1], embedding_scale=7.5)
        # Guidance returns 7.5 out - 6.5 out_masked (modules.py:1248-1253) of two passes.  Exact-fp32 products hold the 1e-4 contract on
        # this raw network output too.  Split-bf16: each pass is within 5e-5 (asserted above), so the mix is within 14 x 5e-5 = 7e-4 in the
        # worst case and 7.5 x 5e-5 = 3.75e-4 when the two passes' errors are alike; measured 0.4e-4 .. 2.7e-4 over the seven models.
        # The quantity with a contract is what the sampler consumes -- c_skip x + c_out net(), asserted at 1e-4 for every mode below.
        bound = 1e-4 if models.mode == "f32" else 4e-4
        assert (y.cpu() - to_t(g["y_scale7p5"])[b:b + 1]).abs().max() < bound, (case, b, models.mode)
    d = m.diffusion.diffusion.denoise_fn(x * 2.5, sigma=torch.tensor(2.5), embedding=emb, embedding_scale=1.0)
    assert (d.cpu() - to_t(g["denoise_sigma2p5"])).abs().max() < 5e-5
    if models.mode == "f32":
        # 'exact fp32' is exact on EVERY fused op (round 6: the C = 256 sub-block kernel k_tblock32 has fp32 instantiations too): no
        # ring-kernel op of an f32 program may carry split-bf16 tiles
        from moleculediffusiontransformer_amd import runtime as rt
        wf = {rt.OP_TF128: rt.F_WF32, rt.OP_TF256: rt.F_WF32, rt.OP_RES256: rt.F_WF32, rt.OP_RCONV: rt.R_WF32, rt.OP_RESBLOCK: rt.K_WF32,
              rt.OP_TBLOCK: rt.B_WF32}
        for name in ("eval", "ctx"):
            assert all(op.i[wf[op.kind]] == 1 for op in m._engine.c.programs[name] if op.kind in wf), (case, name)
    # denoise_fn UNDER GUIDANCE (diffusion.py:798-814 over modules.py:1248-1253) against the reference: the 1e-4 contract, all modes
    d = m.diffusion.diffusion.denoise_fn(x * 2.5, sigma=torch.tensor(2.5), embedding=emb, embedding_scale=7.5)
    gd = load_golden("guided_denoise.npz")[f"{case}_denoise_sigma2p5_scale7p5"]
    assert (d.cpu() - to_t(gd)).abs().max() < TOL, (case, models.mode)


@pytest.mark.parametrize("name,case,want", [
    ("tiny_b3_t8", "tiny", (1, 7)),
    ("tiny_b3_t8_cfg2", "tiny", ()),
    ("pd22_b2_t6", "pd22", ()),
    ("cfg3_b2_t10", "cfg3", ()),
    ("cfg1_b2_t12_cfg7p5", "cfg1", ()),
    ("cfg1_b4_t64", "cfg1", (1, 2, 32, 63)),
    ("nb_b2_t6", "nb", ()),              # the notebook's trained configuration (Inverse_Diffusion.ipynb:1587-1604)
    ("nb_b2_t5_cfg2", "nb", ()),
    ("sparse_b2_t5", "sparse", ()),      # AnalogDiffusionSparse-shaped U-Net (graphmodel.py:266-283)
    ("full_b2_t5", "full", ()),          # AnalogDiffusionFull with pos_emb_fourier_add=True (graphmodel.py:391-597)
    ("full_b2_t4_cfg3", "full", ()),
])
def test_sample_matches_reference(models, name, case, want):
    g = load_golden(f"{name}_sample.npz")
    m = models(case)
    out_ref = to_t(g["out"])
    init, step = noise_fns(name, tuple(out_ref.shape))
    trace = {"want": want}
    out = m.sample(to_t(g["seq"]), DEV, cond_scale=float(g["cond_scale"]), timesteps=int(g["timesteps"]), clamp=False,
                   noise=NoiseSource(init=init, steps=lambda i: step(i, init)), trace=trace)
    assert out.shape == out_ref.shape and out.device.type == "cuda" and not out.requires_grad
    for s in want:
        assert (trace[s].cpu() - to_t(g[f"x_step{s}"])).abs().max() < TOL, (name, s)
    assert (out.cpu() - out_ref).abs().max() < TOL


def _switch_cases():
    from test_host_logic import FALLBACK_SWITCHES
    return [pytest.param(var, value, case, id=f"{var}={value}-{case}") for var, value, cases in FALLBACK_SWITCHES for case in cases]      # ("case+VAR=v": on top of that fallback)


@pytest.mark.parametrize("var,value,case", _switch_cases())
def test_every_fallback_switch_matches_reference(var, value, case, monkeypatch):
    """every MDT_* switch that turns a fused form back into its previous form is FLIPPED here and
    the program it selects evaluated on the GPU against the reference's golden U-Net output (CPU half:
    tests/test_host_logic.py::test_every_fallback_switch_lowers_to_the_reference_result) -- a switch nobody flips is a dead
    configuration.  MDT_B16 / MDT_QKV_MERGE belong to the reduced-precision mode (budget 2e-2 per evaluation)."""
    monkeypatch.setenv(var, value)
    monkeypatch.setenv("MDT_F32_FUSED", "1")
    case, _, under = case.partition("+")
    if under:
        monkeypatch.setenv(*under.split("="))
    g = load_golden(f"{case}_unet.npz")
    m = make_model(case)
    bf16 = var in ("MDT_B16", "MDT_QKV_MERGE", "MDT_RES16", "MDT_LNFOLD", "MDT_CAT_FOLD")
    if bf16:
        m.gemm_mode = "bf16"
    emb = m._embed(to_t(g["seq"]), DEV)
    x, t = to_t(g["x"]).to(DEV), to_t(g["t"])
    scale = 2.0 if var == "MDT_CFG_DUAL" else 1.0                 # (the dual / two-pass choice exists under guidance only)
    want = to_t(g["y_scale1"])
    for b in range(x.shape[0]):
        y = m.unet(x[b:b + 1], t[b:b + 1], embedding=emb[b:b + 1], embedding_scale=1.0)
        assert (y.cpu() - want[b:b + 1]).abs().max() < (2e-2 if bf16 else 5e-5), (var, value, case, b)
    if scale != 1.0:
        name = "cfg1_b2_t12_cfg7p5"
        gs = load_golden(f"{name}_sample.npz")
        init, step = noise_fns(name, tuple(gs["out"].shape))
        out = m.sample(to_t(gs["seq"]), DEV, cond_scale=7.5, timesteps=int(gs["timesteps"]), clamp=False,
                       noise=NoiseSource(init=init, steps=lambda i: step(i, init)))
        assert not m._engine.has_dual and (out.cpu() - to_t(gs["out"])).abs().max() < TOL
    assert m._engine.handoff_status() == 0


@pytest.mark.parametrize("mode", ["bf16x3", "f32"])
def test_chained_resnet_blocks_match_the_reference_sample(mode, monkeypatch):
    """MDT_OP_RES256 forced on (MDT_RES256=1) in the NARROW program of configs[1] -- the automatic policy uses it in the wide program
    and on one-token levels only -- against the reference's 64-step golden sample with its intermediate sampler states, both
    product types; 20 launches per evaluation."""
    from moleculediffusiontransformer_amd import runtime as rt
    monkeypatch.setenv("MDT_RES256", "1")
    monkeypatch.setenv("MDT_F32_FUSED", "1")
    g = load_golden("cfg1_b4_t64_sample.npz")
    m = make_model("cfg1")
    m.gemm_mode = mode
    out_ref = to_t(g["out"])
    init, step = noise_fns("cfg1_b4_t64", tuple(out_ref.shape))
    trace = {"want": (1, 2, 32, 63)}
    out = m.sample(to_t(g["seq"]), DEV, cond_scale=1.0, timesteps=64, clamp=False,
                   noise=NoiseSource(init=init, steps=lambda i: step(i, init)), trace=trace)
    ops = m._engine.c.programs["eval"]
    kinds = [op.kind for op in ops]
    # (the only MDT_OP_RCONV launches left are the four resampling convolutions in patch form: half-output / K-block / output-block ops)
    rc = [op for op in ops if op.kind == rt.OP_RCONV]
    assert kinds.count(rt.OP_RES256) == 4 and len(kinds) == 20
    assert len(rc) == 4 and all(op.i[rt.R_HALF_OUT] or op.i[rt.R_KSRC] or op.i[rt.R_NB] for op in rc) and rt.OP_GEMM not in kinds
    for s_ in (1, 2, 32, 63):
        assert (trace[s_].cpu() - to_t(g[f"x_step{s_}"])).abs().max() < TOL, s_
    assert (out.cpu() - out_ref).abs().max() < TOL


def test_wide_batch_kernel_choice_matches_reference():
    """The 256-channel transformers run pair-split (k_tf256 NSPLIT = 2) at small batches and as whole-transformer launches without the
    split above 4096 rows at that level, 1024 samples here (generative.py::_wide).  Both forms against the reference's golden sample, the automatic
    choice by batch size, and the pin that makes per-sample results independent of how a batch is sharded."""
    from moleculediffusiontransformer_amd import runtime as rt
    g = load_golden("cfg1_b2_t12_cfg7p5_sample.npz")
    m = make_model("cfg1")
    seq, T = to_t(g["seq"]), int(g["timesteps"])
    init, step = noise_fns("cfg1_b2_t12_cfg7p5", tuple(g["out"].shape))
    outs = {}
    for choice in ("narrow", "wide"):
        m.kernel_choice = choice
        outs[choice] = m.sample(seq, DEV, cond_scale=7.5, timesteps=T, noise=NoiseSource(init=init, steps=lambda i: step(i, init))).cpu()
        forms = {op.i[rt.F_NSPLIT] for op in m._engine.c.programs["eval"] if op.kind == rt.OP_TF256}
        assert forms == ({1} if choice == "wide" else {2}) and m._engine.c.tf256 == (choice == "wide")
        # round 5: the wide program chains the 256-channel level's ResNet blocks (MDT_OP_RES256: 4 launches instead of 26)
        kinds = [op.kind for op in m._engine.c.programs["eval"]]
        # ... and since round 6 the narrow program too, as PAIR-SPLIT chains (k_res256 NSPLIT = 2, hand-offs inside the launch)
        assert len(kinds) == 20 and kinds.count(rt.OP_RES256) == 4
        assert {op.i[rt.F_NSPLIT] for op in m._engine.c.programs["eval"] if op.kind == rt.OP_RES256} == ({0} if choice == "wide" else {2})
        assert m._engine.handoff_status() == 0
        assert (outs[choice] - to_t(g["out"])).abs().max() < TOL
    m.kernel_choice = "auto"
    assert m._wide(1024) is False and m._wide(1032) is True and m._wide(2048) is True and m._wide(None) is False


def test_kernel_choice_pin_makes_shards_bitwise_equal_across_the_threshold():
    """2048 samples on one rank take the wide form, 2 x 1024 on two ranks the narrow one, and the two forms agree
    to rounding only.  With the choice pinned from the largest shard (distributed.pin_for_shards, what sample_sharded(model=)
    does) a 1-rank run of any sub-batch reproduces the sharded rows bit for bit; unpinned ('auto') it is tolerance only."""
    from moleculediffusiontransformer_amd.distributed import pin_for_shards
    m = make_model("cfg1")
    B, T = 2048, 3
    seq = synth_normal("straddle/seq", (B, 12))
    run = lambda s, first: m.sample(s, DEV, cond_scale=1.0, timesteps=T, noise=NoiseSource(seed=77, sample0=first))   # noqa: E731
    assert m.kernel_choice == "auto"
    whole_auto = run(seq, 0)                       # 2048 rows: wide
    assert m._engine.c.tf256
    assert pin_for_shards(m, B, 2) == "narrow"     # two shards of 1024
    halves = torch.cat([run(seq[:1024], 0), run(seq[1024:], 1024)])
    assert not m._engine.c.tf256
    whole_pinned = run(seq, 0)                     # the 1-rank run with the same pin: same kernels at 2048 rows
    assert not m._engine.c.tf256
    assert torch.equal(whole_pinned, halves)
    assert (whole_auto - halves).abs().max() < 1e-4
    m.pin_kernel_choice(None)
    assert m.kernel_choice == "auto"


def test_inpaint_matches_reference(models):
    g = load_golden("tiny_inpaint.npz")
    m = models("tiny")
    src, mask = to_t(g["src"]), to_t(g["mask"])
    n = {"i": 0}

    def draw():
        t = synth_normal(f"tiny_inpaint/draw{n['i']}", tuple(src.shape))
        n["i"] += 1
        return t
    out = m.inpaint(to_t(g["seq"]), DEV, cond_scale=float(g["cond_scale"]), timesteps=int(g["timesteps"]),
                    num_resamples=int(g["num_resamples"]), inpaint=src.to(DEV), in_paint_mask=mask.to(DEV), draw=draw)
    assert n["i"] == int(g["ndraws"])
    assert (out.cpu() - to_t(g["out"])).abs().max() < TOL
    assert torch.equal(out.cpu()[mask], src[mask])


def test_batch64_against_oracle_and_graph_replay_is_bitwise_identical(models):
    """A batch larger than any golden fixture, checked against the (pinned) oracle on identical noise;
    HIP-graph replay and plain launches must agree bit for bit."""
    m = models("cfg1")
    B, T = 64, 6
    seq = synth_normal("b64/seq", (B, 12))
    init = synth_normal("b64/init", (B, 16, 64))
    steps = [synth_normal(f"b64/step{i}", (B, 16, 64)) for i in range(T - 1)]
    ref = O.sample(synth_sd("cfg1"), oracle_cfg("cfg1"), seq, init, lambda i, x: steps[i], T, 1.0, True)
    outs = []
    for use_graph in (True, False):
        eng = m.engine(DEV, 12)
        eng.use_graph = use_graph
        eng._graphs.clear()
        outs.append(m.sample(seq, DEV, cond_scale=1.0, timesteps=T, clamp=True,
                             noise=NoiseSource(init=init, steps=lambda i: steps[i])).cpu())
    assert torch.equal(outs[0], outs[1])
    assert (outs[0] - ref).abs().max() < TOL


def test_seeded_sampling_is_reproducible_and_shard_invariant(models):
    m = models("tiny")
    seq = synth_normal("shard/seq", (8, 12))
    full = m.sample(seq, DEV, cond_scale=1.0, timesteps=5, noise=NoiseSource(seed=99, sample0=0)).cpu()
    again = m.sample(seq, DEV, cond_scale=1.0, timesteps=5, noise=NoiseSource(seed=99, sample0=0)).cpu()
    assert torch.equal(full, again)
    lo = m.sample(seq[:4], DEV, cond_scale=1.0, timesteps=5, noise=NoiseSource(seed=99, sample0=0)).cpu()
    hi = m.sample(seq[4:], DEV, cond_scale=1.0, timesteps=5, noise=NoiseSource(seed=99, sample0=4)).cpu()
    assert torch.equal(torch.cat([lo, hi]), full)
    assert torch.isfinite(full).all()


def test_guidance_as_one_doubled_batch_equals_two_passes(models):
    """cond_scale != 1: both passes of UNetCFG1d.forward (modules.py:1248-1253) run as ONE evaluation of the batch
    [samples | samples] whose second half attends to the FixedEmbedding's K/V (program "eval_dual").  Same kernels, same
    per-row arithmetic: bitwise equal to the two-pass form; B = 12 (not a multiple of 8) takes the two-pass form."""
    m = models("cfg1")
    seq = synth_normal("dual/seq", (16, 12))
    eng = m.engine(DEV, 12)
    if not eng.has_dual:
        pytest.skip("layer-by-layer program (exact-fp32 mode): no dual-batch form")
    one = m.sample(seq, DEV, cond_scale=2.0, timesteps=4, noise=NoiseSource(seed=11, sample0=0)).cpu()
    dual_prog = eng.programs.pop("eval_dual")
    try:
        two = m.sample(seq, DEV, cond_scale=2.0, timesteps=4, noise=NoiseSource(seed=11, sample0=0)).cpu()
    finally:
        eng.programs["eval_dual"] = dual_prog
    assert torch.isfinite(one).all() and torch.equal(one, two)
    part = m.sample(seq[:12], DEV, cond_scale=2.0, timesteps=4, noise=NoiseSource(seed=11, sample0=0)).cpu()
    assert torch.equal(part, one[:12])


def test_default_rng_mode_consumes_cpu_generator_like_the_reference(models):
    m = models("tiny")
    seq = synth_normal("rng/seq", (2, 12))
    torch.manual_seed(7)
    a = m.sample(seq, DEV, cond_scale=1.0, timesteps=4)
    torch.manual_seed(7)
    b = m.sample(seq, DEV, cond_scale=1.0, timesteps=4)
    assert a.shape == (2, 16, 32) and torch.equal(a, b)


def test_cfg5_architecture_against_oracle():
    """BASELINE.json configs[4] shape (channels=256, pred_dim=32, max_len=128; 292.6 M parameters): levels with
    C = 512 / 1024 and 32 tokens per sample run on the generic layer-by-layer kernels.  No golden vector exists
    for this size; the pinned oracle is the reference (fp32 GEMM mode is exercised by the other tests)."""
    m = make_model("cfg5")
    assert sum(p.numel() for p in m.parameters()) == 292622880
    sd, cfg = synth_sd("cfg5"), oracle_cfg("cfg5")
    B, T = 2, 3
    seq = synth_normal("cfg5/seq", (B, 12))
    init = synth_normal("cfg5/init", (B, 32, 128))
    steps = [synth_normal(f"cfg5/step{i}", (B, 32, 128)) for i in range(T - 1)]
    ref = O.sample(sd, cfg, seq, init, lambda i, x: steps[i], T, 1.0, False)
    out = m.sample(seq, DEV, cond_scale=1.0, timesteps=T, clamp=False,
                   noise=NoiseSource(init=init, steps=lambda i: steps[i])).cpu()
    assert (out - ref).abs().max() < TOL
    with torch.no_grad():
        emb = O.cond_embed(sd, cfg, seq)
        x = synth_normal("cfg5/x", (B, 32, 128))
        y_ref = O.unet_forward(sd, cfg, x, torch.full((B,), 0.2), emb)
    y = m.unet(x.to(DEV), torch.full((B,), 0.2), embedding=emb.to(DEV), embedding_scale=1.0).cpu()
    assert (y - y_ref).abs().max() < 1e-4 * max(1.0, y_ref.abs().max().item())


def test_edge_batches_single_and_empty():
    """B = 1 (a lone sample in a 32 / 64-row workgroup: every other row is padding) equals row 0 of a B = 3 run with
    the same per-sample noise; B = 0 returns an empty tensor of the right shape without launching anything."""
    m = make_model("cfg1")
    seq = synth_normal("edge/seq", (3, 12))
    init = synth_normal("edge/init", (3, 16, 64))
    steps = [synth_normal(f"edge/step{i}", (3, 16, 64)) for i in range(5)]
    full = m.sample(seq, DEV, cond_scale=1.0, timesteps=6, clamp=False,
                    noise=NoiseSource(init=init, steps=lambda i: steps[i])).cpu()
    one = m.sample(seq[:1], DEV, cond_scale=1.0, timesteps=6, clamp=False,
                   noise=NoiseSource(init=init[:1], steps=lambda i: steps[i][:1])).cpu()
    assert one.shape == (1, 16, 64) and torch.isfinite(one).all()
    assert torch.equal(one[0], full[0])                 # per-sample arithmetic does not depend on the batch around it
    empty = m.sample(seq[:0], DEV, cond_scale=1.0, timesteps=6, clamp=False, noise=NoiseSource(seed=3))
    assert empty.shape == (0, 16, 64)


def test_bench_plain_line_and_dumped_outputs(tmp_path):
    """A plain bench.py run prints the headline alone (no roofline, no other legs) for exactly --steps timed steps, and
    --dump-outputs writes the samples of the last timed step.  The same arguments with --full (every evaluation HIP-event
    timed, then the extra legs) dump the same bits: the inputs are seeded and both runs compute the same thing."""
    import json
    import os
    import subprocess
    import sys
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env.pop("RANK", None)
    lines = {}
    for leg in ("plain", "full"):
        args = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "64", "--timesteps", "4",
                "--dump-outputs", str(tmp_path / leg)]
        if leg == "full":
            args += ["--full", "--no-breakdown", "--no-cpu-baseline", "--no-exact-f32", "--no-other-configs"]
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), *args],
                           capture_output=True, text=True, timeout=900, env=env, cwd=root)
        assert r.returncode == 0, r.stderr[-3000:]
        out = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(out) == 1, r.stdout[-2000:]
        lines[leg] = json.loads(out[0])
    d = lines["plain"]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 2 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 - 64) < 0.5             # molecules/s x s per step = molecules per step
    assert not {"roofline", "unet_eval", "power", "exact_f32", "other_configs", "cpu_baseline"} & set(d)
    assert {"roofline", "unet_eval"} <= set(lines["full"]) and lines["full"]["unet_eval"]["evals_timed"] == 2 * 6
    a, b = np.load(tmp_path / "plain" / "samples.npy"), np.load(tmp_path / "full" / "samples.npy")
    assert a.shape == (64, 16, 64) and a.dtype == np.float32 and np.isfinite(a).all()
    assert np.array_equal(a, b)


def test_bench_two_rank_logic_on_one_gpu():
    """bench.py's N > 1 path as the driver invokes it (`python bench.py --gpus 2`, no torchrun around it): the script
    launches its own ranks as a child process, barriers, one all-gather per call, max-over-ranks timing, ONE JSON line from
    rank 0, and the gathered rows of the last rank equal a 1-rank run of those global sample indices bit for bit.
    Two ranks share cuda:0 over gloo here (test hook MDT_BENCH_SHARE_GPU; the real thing is one rank per GPU over RCCL)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MDT_BENCH_SHARE_GPU="1")
    env.pop("RANK", None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "1",
                        "--batch", "64", "--timesteps", "4", "--no-breakdown", "--full", "--master-port", "29533"],
                       capture_output=True, text=True, timeout=900, env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["global_batch"] == 128 and d["scaling"] == "weak" and d["value"] > 0
    mg = d["multi_gpu"]
    assert mg["rccl_ranks_seen"] == 2 and mg["gathered_rows"] == 128 and mg["collectives_per_step"] == 1
    assert mg["shard_invariance"]["bitwise_equal_to_1_rank_run"] is True and mg["shard_invariance"]["rank"] == 1
    # round 6: the collective timed apart from the compute, per-rank rates, the N = 1 equivalent
    pr = mg["per_rank_molecules_per_s"]
    assert len(pr["ranks"]) == 2 and len(mg["sample_ms_per_step_per_rank"]) == 2 and 0 < pr["min"] <= mg["n1_equivalent_value"] <= pr["max"]
    assert 0 <= mg["all_gather_ms_per_step"]["min_over_ranks"] <= mg["all_gather_ms_per_step"]["max_over_ranks"]
    assert abs(mg["value_per_gpu"] * 2 - d["value"]) < 0.2 and mg["value_per_gpu"] <= pr["max"] * 1.001


def test_bench_eight_rank_logic_on_one_gpu():
    """the same self-launch path with EIGHT ranks (`python bench.py --gpus 8`), sharing cuda:0 over gloo at a small
    batch: eight children, one JSON line, eight ranks seen by the all-gather, 8 x 32 gathered rows, and the bitwise shard-invariance
    check on the LAST rank's rows (global sample indices 224..255 against a 1-rank run)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MDT_BENCH_SHARE_GPU="1", OMP_NUM_THREADS="2")
    env.pop("RANK", None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "8", "--steps", "1", "--warmup", "1",
                        "--batch", "32", "--timesteps", "3", "--no-breakdown", "--full", "--master-port", "29541"],
                       capture_output=True, text=True, timeout=1500, env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 8 and d["config"]["global_batch"] == 256 and d["scaling"] == "weak" and d["value"] > 0
    mg = d["multi_gpu"]
    assert mg["rccl_ranks_seen"] == 8 and mg["gathered_rows"] == 256 and mg["collectives_per_step"] == 1
    assert mg["shard_invariance"]["bitwise_equal_to_1_rank_run"] is True and mg["shard_invariance"]["rank"] == 7


@pytest.mark.slow
def test_bench_eight_ranks_at_the_configs3_shard_size_on_one_gpu():
    """BASELINE configs[3] EXACTLY as the driver will invoke it -- `python bench.py --gpus 8 --batch 8192` = 65,536
    molecules, the wide program on every rank -- as a dry run with the eight ranks sharing cuda:0 over gloo (test hook; ~10 GB of
    activations per rank).  Not a scaling measurement (the ranks take turns on one GPU): it checks the N > 1 line at the real shard
    size -- global batch, one collective per step, the all-gather timed apart from the compute, eight per-rank rates, the N = 1
    equivalent, bitwise shard invariance of the last rank's rows.  `-m "gpu and slow"` (about a minute)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MDT_BENCH_SHARE_GPU="1", OMP_NUM_THREADS="4")
    env.pop("RANK", None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "8", "--steps", "1", "--warmup", "1",
                        "--batch", "8192", "--no-breakdown", "--full", "--master-port", "29547"],
                       capture_output=True, text=True, timeout=1500, env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 8 and d["config"]["global_batch"] == 65536 and d["config"]["timesteps"] == 64 and d["scaling"] == "weak"
    mg = d["multi_gpu"]
    assert mg["rccl_ranks_seen"] == 8 and mg["gathered_rows"] == 65536 and mg["collectives_per_step"] == 1
    assert mg["all_gather_bytes_per_rank"] == 8192 * 16 * 64 * 4
    assert len(mg["per_rank_molecules_per_s"]["ranks"]) == 8 and mg["n1_equivalent_value"] > 0
    assert mg["shard_invariance"]["bitwise_equal_to_1_rank_run"] is True and mg["shard_invariance"]["rank"] == 7
    assert d["unet_eval"]["launches"] == 20
    out = os.path.join(root, "gpurun_out", "r6")
    if os.path.isdir(os.path.join(root, "gpurun_out")):
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "bench_8ranks_shared_gpu.json"), "w") as f:
            f.write(lines[0] + "\n")


def test_rccl_all_gather_runs_on_one_gpu():
    """the RCCL path had never executed anywhere.  On a one-GPU box: (i) backend "nccl" (= RCCL) at world size 1
    with all_gather_into_tensor FORCED through all_gather_samples / all_gather_tokens on device tensors; (ii) bench.py as one
    rank of a rank environment (RANK=0 WORLD_SIZE=1): process group up, gather per step, barrier + max-over-ranks timing,
    `multi_gpu` in the line with the shard-invariance probe."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = """
import os, torch, torch.distributed as dist
from moleculediffusiontransformer_amd.distributed import all_gather_samples, all_gather_tokens
import moleculediffusiontransformer_amd.ops
dev = torch.device('cuda', 0); torch.cuda.set_device(dev)
dist.init_process_group('nccl', rank=0, world_size=1, device_id=dev)
x = torch.randn(5, 16, 64, device=dev)
y = all_gather_samples(x, 5, force_collective=True)
assert y.data_ptr() != x.data_ptr() and torch.equal(y, x)
t = torch.randint(0, 16, (5, 64), device=dev)
assert torch.equal(all_gather_tokens(t, 5, 16, force_collective=True), t)
z = torch.ops.mdt.all_gather_samples(x, 5)
assert torch.equal(z, x)
dist.barrier(); torch.cuda.synchronize(); dist.destroy_process_group(); print('RCCL_OK', dist.Backend.NCCL)
"""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29541", HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=root)
    env.pop("RANK", None)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env, cwd=root)
    assert r.returncode == 0 and "RCCL_OK" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
    env.update(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_PORT="29542")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1", "--batch", "64",
                        "--timesteps", "4", "--full", "--no-breakdown", "--no-cpu-baseline", "--no-exact-f32", "--no-other-configs"],
                       capture_output=True, text=True, timeout=900, env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    mg = d["multi_gpu"]
    assert d["n_gpus"] == 1 and mg["backend"].startswith("nccl") and mg["rccl_ranks_seen"] == 1 and mg["gathered_rows"] == 64
    assert mg["shard_invariance"]["bitwise_equal_to_1_rank_run"] is True


@pytest.mark.parametrize("mode", ["bf16x3", "f32"])
@pytest.mark.parametrize("B,cs", [(8, 1.0), (256, 1.0), (1024, 1.0), (256, 3.0)])
def test_repeated_sampling_is_bitwise_stable(B, cs, mode, monkeypatch):
    """The same call six times on identical noise returns identical bits, and the probe rows match the oracle -- with launches of
    DIFFERENT data alternating (evaluations of a sampling loop), which an op-level repeat on fixed inputs cannot exercise.  This is
    the check that exposed the first form of the pair hand-off (wave-uniform part of the addresses in the buffer instructions'
    SCALAR offset: a piece in 10^5-10^7 arrived from another block; B = 1024 differed in every call; DESIGN.md 3.8,
    tools/repeat_determinism_probe.py)."""
    monkeypatch.setenv("MDT_F32_FUSED", "1")     # (the module-scoped `models` fixture of the layer-by-layer form may still be alive)
    m = make_model("cfg1")
    m.gemm_mode = mode                 # 'f32': the same fused program (pair hand-offs included) with exact fp32 products
    T = 3 if B < 1024 else 2
    seq = synth_normal("rep/seq", (B, 12))
    init = synth_normal("rep/init", (B, 16, 64))
    nz = [synth_normal(f"rep/s{i}", (B, 16, 64)) for i in range(T - 1)]
    rows = torch.tensor(sorted({0, 1, B // 2, B - 1}))
    want = O.sample(synth_sd("cfg1"), oracle_cfg("cfg1"), seq[rows], init[rows], lambda i, x: nz[i][rows], T, cs, False)
    outs = [m.sample(seq, DEV, cond_scale=cs, timesteps=T, noise=NoiseSource(init=init, steps=lambda i: nz[i])) for _ in range(6)]
    assert all(torch.equal(outs[0], o) for o in outs[1:])
    assert (outs[0].cpu()[rows] - want).abs().max() < TOL
    assert m._engine.handoff_status() == 0
    from moleculediffusiontransformer_amd import runtime as rt
    ev = m._engine.c.programs["eval"]
    assert len(ev) == 20 and all(op.i[rt.F_WF32] == int(mode == "f32") for op in ev if op.kind in (rt.OP_TF128, rt.OP_TF256, rt.OP_RES256))
    assert all(op.i[rt.F_NSPLIT] == 2 for op in ev if op.kind in (rt.OP_TF256, rt.OP_RES256))      # narrow program: every 256-channel launch pair-split


def test_handoff_timeout_is_reported_before_the_call_returns():
    """A pair hand-off that times out leaves garbage rows and raises bit 0 of the engine's diagnostic word on the device.  Every
    sampling call copies that word to pinned host memory behind its last launch and WAITS for it before returning (VERDICT r3:
    a caller who samples once and uses the tensor must learn); with model.defer_handoff_check the look moves to the next call.
    The time-out itself is simulated here by setting the word (the real thing: the next test)."""
    m = make_model("cfg1")
    seq = synth_normal("to/seq", (64, 12))
    first = m.sample(seq, DEV, cond_scale=1.0, timesteps=2, noise=NoiseSource(seed=3))
    eng = m._engine
    if eng.xflags is None:
        pytest.skip("no pair-split launch in this program")
    assert eng.sync_handoff_check and not getattr(eng, "_xstat_pending", False)      # the clean call was checked before it returned
    eng.xflags[0] = 1                                 # what a timed-out poll does (sticky until reported)
    with pytest.raises(RuntimeError, match="results of this call are invalid"):
        m.sample(seq, DEV, cond_scale=1.0, timesteps=2, noise=NoiseSource(seed=3))
    assert eng.handoff_status() == 0                  # reported once, cleared
    again = m.sample(seq, DEV, cond_scale=1.0, timesteps=2, noise=NoiseSource(seed=3))
    assert torch.equal(first, again)
    # net(x, t) / denoise_fn evaluations are checked the same way (they never looked at the word)
    eng.xflags[0] = 1
    emb = m._embed(seq, DEV)
    with pytest.raises(RuntimeError, match="pair hand-off"):
        m.unet(torch.zeros(64, 16, 64, device=DEV), torch.tensor(0.5), embedding=emb, embedding_scale=1.0)
    # the opt-out for pipelined callers: the failed call returns, the NEXT one raises
    m.defer_handoff_check = True
    m.sample(seq, DEV, cond_scale=1.0, timesteps=2, noise=NoiseSource(seed=3))
    assert not m._engine.sync_handoff_check
    m._engine.xflags[0] = 1
    m.sample(seq, DEV, cond_scale=1.0, timesteps=2, noise=NoiseSource(seed=3))       # returns: deferred
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="PREVIOUS call"):
        m.sample(seq, DEV, cond_scale=1.0, timesteps=2, noise=NoiseSource(seed=3))
    m.defer_handoff_check = False


def test_pair_split_launch_without_co_residency_fails_loudly_or_is_correct():
    """The real thing: a kernel on a SECOND stream holds all but two compute units for 1.2 s (mdt_test_occupy:
    160 KiB of LDS per workgroup, nothing fits next to it) while a 1024-sample call with pair-split launches (256 workgroups, the
    partners 8 ids apart) is enqueued.  The first workgroups to run do not find their partners resident, their polls give up after
    0.3 s and leave garbage.  Whatever the interleaving: sample() either raises RuntimeError before returning or returns the
    bits of an undisturbed call -- never silent garbage."""
    from moleculediffusiontransformer_amd import runtime as rt
    lib = rt.load_library()
    m = make_model("cfg1")
    m.kernel_choice = "narrow"
    B = 1024
    seq = synth_normal("hog/seq", (B, 12))
    run = lambda: m.sample(seq, DEV, cond_scale=1.0, timesteps=2, noise=NoiseSource(seed=5))   # noqa: E731
    clean = run()
    assert any(op.kind == rt.OP_TF256 and op.i[rt.F_NSPLIT] == 2 for op in m._engine.c.programs["eval"])
    cap = rt.pair_capacity()
    assert cap >= 64
    side = torch.cuda.Stream(device=DEV)
    outcomes = []
    for hold in (cap - 2, cap - 16):
        with torch.cuda.device(DEV):
            rt.check(lib.mdt_test_occupy(hold, 160 * 1024, 120_000_000, side.cuda_stream))      # 1.2 s
        try:
            out = run()
            outcomes.append("ok")
            assert torch.equal(out, clean), "a disturbed call returned without an error AND with different bits"
        except RuntimeError as e:
            assert "pair hand-off" in str(e)
            outcomes.append("raised")
        torch.cuda.synchronize()
    assert m._engine.handoff_status() == 0                 # nothing left unreported
    assert torch.equal(run(), clean)                       # and the engine is usable afterwards
    print("outcomes with the device held:", outcomes)


def test_pair_split_batch_larger_than_the_device_runs_in_chunks():
    """a pinned 'narrow' kernel choice used to put 2 x ceil(rows / 32) workgroups into ONE launch whatever the batch --
    beyond the device's co-residency capacity forward progress hung on dispatch order.  launch_tf256 now asks the device
    (mdt_pair_capacity = compute units x occupancy) and splits such a batch into launches that fit; here the capacity is forced
    down to 32 workgroups (mdt_set_tuning) so that B = 64 (8 row blocks, 16 workgroups per launch at stride 8 -> 2 per launch...)
    runs in several launches: same bits as the single launch, flags count as before."""
    from moleculediffusiontransformer_amd import runtime as rt
    lib = rt.load_library()
    m = make_model("cfg1")
    m.kernel_choice = "narrow"
    B = 200                                                # 800 rows = 25 row blocks at the 256-channel level
    seq = synth_normal("chunk/seq", (B, 12))
    run = lambda: m.sample(seq, DEV, cond_scale=1.0, timesteps=3, noise=NoiseSource(seed=11))   # noqa: E731
    assert rt.pair_capacity() >= 64
    one = run()
    try:
        assert lib.mdt_set_tuning(b"pair_capacity", 16) == 0          # one group of 2 x 8 workgroups per launch: 4 launches
        assert rt.pair_capacity() == 16
        m._engine._graphs.clear()                                      # re-capture with the chunked launches
        many = run()
        assert lib.mdt_set_tuning(b"pair_capacity", 8) == 0           # not even one group fits: refused, loudly
        m._engine._graphs.clear()
        with pytest.raises(RuntimeError, match="launch failed"):
            run()
    finally:
        lib.mdt_set_tuning(b"pair_capacity", 0)
        m._engine._graphs.clear()
    assert torch.equal(one, many)
    m.kernel_choice = "auto"
    assert m._wide(1024) is False and m._wide(1025) is True           # 'auto' follows the device's capacity (256 on an MI355X)
