"""-m gpu: results must not depend on memory that no operand owns (harness: tests/poison_util.py).

(a) Operators.  The cases of tests/test_gpu_ops.py below are re-run with that module's run_both replaced by check_poisoned on the
C-ABI runner: every buffer sits between guard bands, everything outside the interpreter's footprint (weights included) holds zeros,
then NaN, then large finite garbage; owned floats must not change with the fill, nobody's floats must come back bit for bit.  The
test functions' own assertions against the interpreter and the closed forms still run, on the baseline.  `prod`: the ring kernels
with split-bf16 and with exact-fp32 tiles.  Tuples: the smallest of each parametrisation with a row count B R that is no multiple
of 16 / 32 / 64, a key count that is no multiple of 16, a channel count below the padded one; for k_gn_act one shape per reachable
dispatch branch of launch_gn_act.

  function (test_gpu_ops.py)                            tuples
  ----------------------------------------------------  ------------------------------------------------------------------------
  test_gemm_plain_bias_gelu_residual                    (7,16,48,32,1) (1,1,80,256,1) (5,64,16,64,3)
  test_row_stationary_projection_on_ring_tiles  [prod]  (37,1,256,1024) (5,4,128,64) x ln/res ("plain",True) ("affine",False)
  test_row_stationary_conv_as_a_k1024_projection [prod] (37,2,256,res) (5,16,128,no res)
  test_strided_convolution_in_patch_form        [prod]  (37,64,64,128,4) (9,4,128,256,4) (5,8,128,256,4)
  test_transposed_convolution_in_patch_form     [prod]  (37,4,256,128,4,res) (9,1,256,128,4,no res) (5,8,128,64,4,res)
  test_gemm_strided_conv_and_transposed_phases          (its one case)
  test_gemm_layernorm_prologue                          (3,12,128,1024) (130,1,64,64)
  test_gn_stats_and_groupnorm_prologue                  (5,4,512,8,256,film,silu) (3,64,64,1,64,silu) (2,32,32,32,32)
  test_attention                                        (2,16,12,per-sample) (2,4,12,shared) (1,100,70: k_attn_long)
  test_attention_with_bf16_operands                     (3,32,12,shared,in16 2,out16 1) (2,8,8,in16 3: merged,out16 0) (1,100,70,in16 3,out16 1)
  test_attention_on_normalised_context                  (2,1,33) split 0 / 1, (5,4,40,split 1), (3,5,64,shared,split 0)
  test_concat_patch_time_embed                          (its one case)
  test_gemm_split_bf16                                  (3,16,128,96,3,GN) (33,1,256,160,1,SiLU) (40,4,256,256,1,GN: A-stationary)
  test_gemm_plain_bf16                                  (3,16,128,96,3,GN) (33,1,256,160,1,SiLU) (5,64,32,64,3,none)
  test_gemm_bf16_streamed                               (5,32,64,96,3,SiLU) tile "" / "1", (3,128,256,256,1,none) tile "2"
  test_gemm_bf16_chain_with_bf16_intermediate           (its one case)
  test_bf16_residual_stream_ops                         (130,4,64,tile -1,w16) (5,32,512,tile 1,w16) (130,4,64,tile 0,generic)
  test_layernorm_folded_into_bf16_gemm                  (67,2,64,128,tile -1) (130,4,256,768,tile 2)
  test_bf16_gemm_bf16_output_into_a_column_block        (plain,w16) (folded,w16) (plain,generic)
  test_bf16_gemm_single_chunk_with_bf16_residual        tile -1, 2
  test_fused_transformer_sub_block                      (256,4,37,variant 2) (128,1,70,variant 0; CROSS: 128,16,5) x FF / SELF / CROSS x bf16x3 / f32
  test_gn_act                                           <1> (2,4,256,32)  <2> (3,16,128,8)  <4> (5,64,64,1)  <8> (2,64,128,1)
                                                        grid<1> (2,16,512,8)  grid<2> (3,32,512,8)  grid<4> (2,32,1024,8)
                                                        grid<8> (2,128,256,4)  <4,1024> (3,32,512,32)  <8,1024> (2,48,512,32)
                                                        (<16> / <32> cannot be reached: 256 % groups == 0 implies 1024 % groups == 0)
  test_gn_act_on_two_sources_with_raw_copy              (3,4,64,4) (37,8,1024,8)
  test_row_stationary_conv_two_sources          [prod]  (256,4,37,3,64) (256,4,9,1,0) (128,16,5,1,0)
  test_row_stationary_conv                      [prod]  (128,16,5,3,16,film,"other") (256,4,9,3,64,"accumulate") (256,1,33,3,32)
  test_fused_resnet_block                       [prod]  (5,50) (2,16) at B = 7 with FiLM, (16,1) at B = 1
  test_fused_resnet_block_with_folded_patch_rearranges [prod]  (2,16,1,2,B 7) (16,8,4,1,B 1) (16,64,1,4,B 7)
  test_chained_split_sub_block                  [prod]  (SELF,split,p_in,4,37) (CROSS,split,p_in,4,37) (FF,no split,no p_in,16,3)
  test_fused_transformer                        [prod]  (256,4,37,2,cross) whole / pair8, (128,2,33,1) (128,16,3,2,cross,fixed) whole
  test_pair_handoff_is_placement_independent_and_repeatable [prod]  (4,37,1,cross)
  test_resnet_blocks_inside_the_transformer_launch [prod]  (1,4,18,2,1) (2,8,9,2,1) (2,16,33,1,1,cross)
  test_resnet_chain_256                         [prod]  whole (1,1,37,2), pair8 (2,8,5,2), pair1 (1,4,70,1)

The 2100-to-8200-row tuples are left to test_gpu_ops.py.  MDT_OP_TBLOCK variant 3 is not re-run: it uses `out` as partial-sum
scratch, which the interpreter does not model (it would count as a store to memory nobody owns).

(b) Engines.  UNetEngine.reserve() is wrapped: whenever it reallocates, the activation arena, the per-row FiLM table and the pair
hand-off buffer -- the three torch.empty allocations -- are filled with the current fill, which is exactly the state torch.empty may
leave.  Every case runs on zeros (baseline), NaN and garbage with a reallocation forced before each run; outputs are bit-equal to the
baseline and finite, handoff_status() is 0; then, without reallocating, other inputs and the first inputs again: the third result
equals the first bit for bit.
"""
import types

import pytest
import torch

import test_gpu_ops as ops_cases
from gpu_util import DEV, make_model
from moleculediffusiontransformer_amd import NoiseSource, runtime as rt
from moleculediffusiontransformer_amd.engine import UNetEngine
from moleculediffusiontransformer_amd.synth import synth_normal
from poison_util import GARBAGE, NAN, ZERO, check_poisoned, gpu_run, poison_
from test_gpu_ops import prod      # noqa: F401  (fixture: split-bf16 / exact-fp32 ring tiles)

pytestmark = pytest.mark.gpu

FF, SELF, CROSS = rt.TB_FF, rt.TB_SELF, rt.TB_CROSS
GN, SILU, NONE = rt.PRO_GROUPNORM, rt.PRO_SILU, rt.PRO_NONE

PLAIN_CASES = [
    ("test_gemm_plain_bias_gelu_residual", (7, 16, 48, 32, 1)),
    ("test_gemm_plain_bias_gelu_residual", (1, 1, 80, 256, 1)),
    ("test_gemm_plain_bias_gelu_residual", (5, 64, 16, 64, 3)),
    ("test_gemm_strided_conv_and_transposed_phases", ()),
    ("test_gemm_layernorm_prologue", (3, 12, 128, 1024)),
    ("test_gemm_layernorm_prologue", (130, 1, 64, 64)),
    ("test_gn_stats_and_groupnorm_prologue", (5, 4, 512, 8, 256, True, True, 1e-5)),
    ("test_gn_stats_and_groupnorm_prologue", (3, 64, 64, 1, 64, False, True, 1e-5)),
    ("test_gn_stats_and_groupnorm_prologue", (2, 32, 32, 32, 32, False, False, 1e-6)),
    ("test_attention", (2, 16, 12, False)),
    ("test_attention", (2, 4, 12, True)),
    ("test_attention", (1, 100, 70, False)),
    ("test_attention_with_bf16_operands", (3, 32, 12, True, 2, 1)),
    ("test_attention_with_bf16_operands", (2, 8, 8, False, 3, 0)),
    ("test_attention_with_bf16_operands", (1, 100, 70, False, 3, 1)),
    ("test_attention_on_normalised_context", (2, 1, 33, False, 0)),
    ("test_attention_on_normalised_context", (2, 1, 33, False, 1)),
    ("test_attention_on_normalised_context", (5, 4, 40, False, 1)),
    ("test_attention_on_normalised_context", (3, 5, 64, True, 0)),
    ("test_concat_patch_time_embed", ()),
    ("test_gemm_split_bf16", (3, 16, 128, 96, 3, GN)),
    ("test_gemm_split_bf16", (33, 1, 256, 160, 1, SILU)),
    ("test_gemm_split_bf16", (40, 4, 256, 256, 1, GN)),
    ("test_gemm_plain_bf16", (3, 16, 128, 96, 3, GN)),
    ("test_gemm_plain_bf16", (33, 1, 256, 160, 1, SILU)),
    ("test_gemm_plain_bf16", (5, 64, 32, 64, 3, NONE)),
    ("test_gemm_bf16_streamed", (5, 32, 64, 96, 3, SILU, 0, "")),
    ("test_gemm_bf16_streamed", (5, 32, 64, 96, 3, SILU, 0, "1")),
    ("test_gemm_bf16_streamed", (3, 128, 256, 256, 1, NONE, 0, "2")),
    ("test_gemm_bf16_chain_with_bf16_intermediate", ()),
    ("test_bf16_residual_stream_ops", (130, 4, 64, -1, 1)),
    ("test_bf16_residual_stream_ops", (5, 32, 512, 1, 1)),
    ("test_bf16_residual_stream_ops", (130, 4, 64, 0, 0)),
    ("test_layernorm_folded_into_bf16_gemm", (67, 2, 64, 128, -1)),
    ("test_layernorm_folded_into_bf16_gemm", (130, 4, 256, 768, 2)),
    ("test_bf16_gemm_bf16_output_into_a_column_block", (False, 1)),
    ("test_bf16_gemm_bf16_output_into_a_column_block", (True, 1)),
    ("test_bf16_gemm_bf16_output_into_a_column_block", (False, 0)),
    ("test_bf16_gemm_single_chunk_with_bf16_residual", (-1,)),
    ("test_bf16_gemm_single_chunk_with_bf16_residual", (2,)),
] + [("test_fused_transformer_sub_block", (mode, C, T, B, variant, products))
     for mode in (FF, SELF, CROSS) for products in ("bf16x3", "f32")
     # (variant 0 serves cross blocks with at most 16 keys per 16 rows: 12 keys need whole 16-token samples)
     for (C, T, B, variant) in ((256, 4, 37, 2), (128, 16, 5, 0) if mode == CROSS else (128, 1, 70, 0))] + [
    ("test_gn_act", (2, 4, 256, 32, False, False, 1e-6)),         # k_gn_act<1>
    ("test_gn_act", (3, 16, 128, 8, True, True, 1e-5)),           # <2>
    ("test_gn_act", (5, 64, 64, 1, False, True, 1e-5)),           # <4>
    ("test_gn_act", (2, 64, 128, 1, False, True, 1e-5)),          # <8>
    ("test_gn_act", (2, 16, 512, 8, True, True, 1e-5)),           # one workgroup per (sample, group): <1, 256, true>
    ("test_gn_act", (3, 32, 512, 8, True, True, 1e-5)),           # <2, 256, true>
    ("test_gn_act", (2, 32, 1024, 8, False, True, 1e-5)),         # <4, 256, true>
    ("test_gn_act", (2, 128, 256, 4, False, True, 1e-5)),         # <8, 256, true>
    ("test_gn_act", (3, 32, 512, 32, False, False, 1e-6)),        # <4, 1024>
    ("test_gn_act", (2, 48, 512, 32, False, False, 1e-6)),        # <8, 1024>
    ("test_gn_act_on_two_sources_with_raw_copy", (3, 4, 64, 4)),
    ("test_gn_act_on_two_sources_with_raw_copy", (37, 8, 1024, 8)),
]

RING_CASES = [      # ... these take the `prod` fixture as their last argument
    ("test_row_stationary_projection_on_ring_tiles", (37, 1, 256, 1024, "plain", True)),
    ("test_row_stationary_projection_on_ring_tiles", (37, 1, 256, 1024, "affine", False)),
    ("test_row_stationary_projection_on_ring_tiles", (5, 4, 128, 64, "plain", True)),
    ("test_row_stationary_projection_on_ring_tiles", (5, 4, 128, 64, "affine", False)),
    ("test_row_stationary_conv_as_a_k1024_projection", (37, 2, 256, True)),
    ("test_row_stationary_conv_as_a_k1024_projection", (5, 16, 128, False)),
    ("test_strided_convolution_in_patch_form", (37, 64, 64, 128, 4)),
    ("test_strided_convolution_in_patch_form", (9, 4, 128, 256, 4)),
    ("test_strided_convolution_in_patch_form", (5, 8, 128, 256, 4)),
    ("test_transposed_convolution_in_patch_form", (37, 4, 256, 128, 4, True)),
    ("test_transposed_convolution_in_patch_form", (9, 1, 256, 128, 4, False)),
    ("test_transposed_convolution_in_patch_form", (5, 8, 128, 64, 4, True)),
    ("test_row_stationary_conv_two_sources", (256, 4, 37, 3, 64, True, 0.7071)),
    ("test_row_stationary_conv_two_sources", (256, 4, 9, 1, 0, False, 0.7071)),
    ("test_row_stationary_conv_two_sources", (128, 16, 5, 1, 0, False, 0.5)),
    ("test_row_stationary_conv", (128, 16, 5, 3, 16, True, True, "other", 1.0)),
    ("test_row_stationary_conv", (256, 4, 9, 3, 64, False, True, "accumulate", 0.7071)),
    ("test_row_stationary_conv", (256, 1, 33, 3, 32, False, True, None, 1.0)),
    ("test_fused_resnet_block", (5, 50, 7, True)),
    ("test_fused_resnet_block", (2, 16, 7, True)),
    ("test_fused_resnet_block", (16, 1, 1, True)),
    ("test_fused_resnet_block_with_folded_patch_rearranges", (2, 16, 1, 2, 7)),
    ("test_fused_resnet_block_with_folded_patch_rearranges", (16, 8, 4, 1, 1)),
    ("test_fused_resnet_block_with_folded_patch_rearranges", (16, 64, 1, 4, 7)),
    ("test_chained_split_sub_block", (SELF, True, True, 4, 37)),
    ("test_chained_split_sub_block", (CROSS, True, True, 4, 37)),
    ("test_chained_split_sub_block", (FF, False, False, 16, 3)),
    ("test_fused_transformer", (256, 4, 37, 2, True, False, "whole")),
    ("test_fused_transformer", (256, 4, 37, 2, True, False, "pair8")),
    ("test_fused_transformer", (128, 2, 33, 1, False, False, "whole")),
    ("test_fused_transformer", (128, 16, 3, 2, True, True, "whole")),
    ("test_pair_handoff_is_placement_independent_and_repeatable", (4, 37, 1, True)),
    ("test_resnet_blocks_inside_the_transformer_launch", (1, 4, 18, 2, 1, False)),
    ("test_resnet_blocks_inside_the_transformer_launch", (2, 8, 9, 2, 1, False)),
    ("test_resnet_blocks_inside_the_transformer_launch", (2, 16, 33, 1, 1, True)),
    ("test_resnet_chain_256", (1, 1, 37, 2, "whole")),
    ("test_resnet_chain_256", (2, 8, 5, 2, "pair8")),
    ("test_resnet_chain_256", (1, 4, 70, 1, "pair1")),
]


def _ids(cases):
    return [f"{name[5:]}-{'-'.join(str(a) for a in args)}" for name, args in cases]


@pytest.fixture
def harness(monkeypatch):
    """test_gpu_ops.run_both -> check_poisoned on the C-ABI runner; counts its calls."""
    seen = types.SimpleNamespace(calls=0)

    def run_both(ops, weights, act, shr, ext, B, n_shr=0):
        seen.calls += 1
        return check_poisoned(gpu_run, ops, weights, act, shr, ext, B, n_shr, device=DEV)
    monkeypatch.setattr(ops_cases, "run_both", run_both)
    return seen


def test_the_tables_cover_every_run_both_test_of_test_gpu_ops():
    import inspect
    users = {n for n, f in vars(ops_cases).items() if n.startswith("test_") and callable(f) and "run_both(" in inspect.getsource(f)}
    listed = {n for n, _ in PLAIN_CASES + RING_CASES}
    assert users == listed, (users - listed, listed - users)
    prod_users = {n for n in users if "prod" in inspect.signature(getattr(ops_cases, n)).parameters}
    assert prod_users == {n for n, _ in RING_CASES}


@pytest.mark.parametrize("name,args", PLAIN_CASES, ids=_ids(PLAIN_CASES))
def test_operator_does_not_depend_on_memory_no_operand_owns(name, args, harness):
    getattr(ops_cases, name)(*args)
    assert harness.calls > 0


@pytest.mark.parametrize("name,args", RING_CASES, ids=_ids(RING_CASES))
def test_ring_operator_does_not_depend_on_memory_no_operand_owns(name, args, harness, prod, monkeypatch):      # noqa: F811
    fn = getattr(ops_cases, name)
    extra = {"monkeypatch": monkeypatch} if name == "test_resnet_chain_256" else {}
    fn(*args, prod=prod, **extra)
    assert harness.calls > 0


# ------------------------------------------------------------------------------------------------------------- (b) engines
HAS_256 = ("cfg1", "sparse")          # cases with a 256-channel level: kernel_choice narrow (pair-split launches, xbuf) and wide


@pytest.fixture
def arena(monkeypatch):
    """reserve() as the contract allows it to behave: whatever it allocates with torch.empty holds the current fill."""
    state = types.SimpleNamespace(fill=ZERO, reallocations=0)
    orig = UNetEngine.reserve

    def reserve(self, B):
        had = self.act
        orig(self, B)
        if self.act is not had and self.B:
            for k, t in enumerate((self.act, self.film, self.xbuf)):
                if t is not None:
                    poison_(t, state.fill, seed=k)
            state.reallocations += 1
    monkeypatch.setattr(UNetEngine, "reserve", reserve)
    return state


@pytest.fixture(scope="module", params=["bf16x3", "f32", "f32-layers"])
def models(request):
    """As tests/test_gpu_parity.py: split-bf16 and exact-fp32 products on the fused program, and the exact mode's layer-by-layer
    form (MDT_F32_FUSED=0, read when an engine is compiled)."""
    import os
    cache = {}
    mode, _, form = request.param.partition("-")
    old = os.environ.get("MDT_F32_FUSED")
    os.environ["MDT_F32_FUSED"] = "0" if form == "layers" else "1"

    def get(case):
        if case not in cache:
            cache[case] = make_model(case)
            cache[case].gemm_mode = mode
        return cache[case]
    get.mode, get.form = mode, form
    yield get
    if old is None:
        del os.environ["MDT_F32_FUSED"]
    else:
        os.environ["MDT_F32_FUSED"] = old


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _drop_arenas(m):
    """Forces the next call to reallocate (and the batch-invariant context to be prepared again, as on a fresh engine)."""
    for eng in m._engines.values():
        eng.reserve(0)
        eng._fixed_ready = False


def under_poison(arena, m, call):
    """call(tag) -> tensor or tuple of tensors, deterministic in tag ('X' / 'Y': two sets of inputs)."""
    def run(tag):
        out = call(tag)
        out = [o.clone() for o in (out if isinstance(out, (tuple, list)) else (out,))]
        torch.cuda.synchronize()
        assert all(eng.handoff_status() == 0 for eng in m._engines.values())
        return out
    outs = {}
    for fill in (ZERO, NAN, GARBAGE):
        arena.fill = fill
        _drop_arenas(m)
        before = arena.reallocations
        outs[fill] = run("X")
        assert arena.reallocations > before, "the call did not reallocate: the poison was not placed"
    base = outs[ZERO]
    assert all(bool(torch.isfinite(o).all()) for o in base if o.is_floating_point())
    for fill in (NAN, GARBAGE):
        for o, b in zip(outs[fill], base):
            assert torch.equal(_bits(o), _bits(b)), f"the result depends on what reserve() allocated ({fill})"
    # history: the arena now holds a poisoned run's leftovers, then another call's, and is not reallocated
    before = arena.reallocations
    other = run("Y")
    third = run("X")
    assert arena.reallocations == before
    assert any(not torch.equal(o, b) for o, b in zip(other, base))
    for o, b in zip(third, base):
        assert torch.equal(_bits(o), _bits(b)), "the result depends on what the previous call left in the arena"


def _inputs(m, tag, B):
    n_seq = m.unet.config.ctx_max_length
    seq = synth_normal(f"poison/{tag}/seq", (B, n_seq))
    x = synth_normal(f"poison/{tag}/x", (B, m.pred_dim, m.max_length)).to(DEV)
    return seq, x


def _denoise(m, B, scale):
    kd = m.diffusion.diffusion

    def call(tag):
        seq, x = _inputs(m, tag, B)
        return kd.denoise_fn(x * 2.5, sigma=torch.tensor(2.5), embedding=m._embed(seq, DEV), embedding_scale=scale)
    return call


def _sample(m, B, scale):
    def call(tag):
        seq, _ = _inputs(m, tag, B)
        return m.sample(seq, DEV, cond_scale=scale, timesteps=3, noise=NoiseSource(seed=7, sample0=0))
    return call


def _dual_batch(m):
    eng = m.engine(DEV, None, 8)
    return max(1, 8 // eng.c.dual_multiple) * eng.c.dual_multiple if eng.has_dual else 8


SHARED_CALLS = {
    "denoise-b1": lambda m: _denoise(m, 1, 1.0),
    "denoise-b3": lambda m: _denoise(m, 3, 1.0),
    "denoise-b37": lambda m: _denoise(m, 37, 1.0),
    "denoise-guided-two-passes-b3": lambda m: _denoise(m, 3, 7.5),            # eval + eval_fixed
    "sample-b3": lambda m: _sample(m, 3, 1.0),
    "sample-guided-dual-b8": lambda m: _sample(m, _dual_batch(m), 7.5),       # eval_dual where the program has it
    "sample-guided-two-passes-b3": lambda m: _sample(m, 3, 7.5),              # 3 is no multiple of dual_multiple (or no eval_dual)
}
ENGINE_CASES = [(case, choice) for case in ("tiny", "pd22", "cfg3", "cfg1", "sparse", "full")
                for choice in (("narrow", "wide") if case in HAS_256 else ("auto",))]


@pytest.mark.parametrize("kind", list(SHARED_CALLS))
@pytest.mark.parametrize("case,choice", ENGINE_CASES, ids=[f"{c}-{k}" for c, k in ENGINE_CASES])
def test_engine_results_do_not_depend_on_what_reserve_allocated(models, arena, case, choice, kind):
    m = models(case)
    old = m.kernel_choice
    m.kernel_choice = choice
    try:
        under_poison(arena, m, SHARED_CALLS[kind](m))
        if kind == "sample-guided-dual-b8":
            eng = m._engine
            assert eng.B == (2 if eng.has_dual else 1) * _dual_batch(m)
        if choice != "auto" and kind == "denoise-b37":
            assert m._engine.c.tf256 == (choice == "wide")
    finally:
        m.kernel_choice = old


@pytest.mark.parametrize("B", [3, 37])
@pytest.mark.parametrize("what", ["denoise-rows", "eval-loss"])
@pytest.mark.parametrize("case", ["tiny", "pd22", "cfg3", "cfg1", "sparse", "full"])
@pytest.mark.parametrize("models", ["bf16x3", "f32"], indirect=True)      # (the same module-scoped models as above)
def test_per_row_engine_results_do_not_depend_on_what_reserve_allocated(models, arena, case, what, B):
    """The per-row engine: activation arena AND the per-sample FiLM table come from torch.empty."""
    m = models(case)
    kd = m.diffusion.diffusion

    def rows(tag):
        seq, x = _inputs(m, tag, B)
        sig = (-1.2 + 1.2 * synth_normal(f"poison/{tag}/sig", (B,))).exp()
        return kd.denoise_fn(x, sigmas=sig, embedding=m._embed(seq, DEV), batched=True)

    def loss(tag):
        seq, x = _inputs(m, tag, B)
        x0 = (0.5 * x).clamp(-1, 1).cpu()
        if getattr(m, "predict_neighbors", False):      # AnalogDiffusionFull: the target is rows 1.. of the packed output
            x0 = torch.cat([torch.zeros(B, 1, m.max_length), x0], dim=1)
        sig = (-1.2 + 1.2 * synth_normal(f"poison/{tag}/sig", (B,))).exp()
        noise = synth_normal(f"poison/{tag}/noise", (B, m.pred_dim, m.max_length))
        return m.eval_loss(seq, x0, DEV, sigmas=sig, noise=noise, per_sample=True)
    under_poison(arena, m, rows if what == "denoise-rows" else loss)
    eng = m._engines[(False, "rows")]
    assert eng.c.rows and eng.film is not None and eng.B == B


@pytest.mark.parametrize("what", ["inpaint-tokens", "refine-tokens"])
def test_token_loops_do_not_depend_on_what_reserve_allocated(models, arena, what):
    m = models("tiny")
    B = 3

    def call(tag):
        seq, _ = _inputs(m, tag, B)
        gen = torch.Generator().manual_seed(11 if tag == "X" else 12)
        draft = torch.randint(0, m.pred_dim, (B, m.max_length), generator=gen)
        if what == "inpaint-tokens":
            keep = torch.rand(B, m.max_length, generator=gen) < 0.4
            return m.inpaint_tokens(seq, DEV, draft, keep, cond_scale=2.0, timesteps=4, num_resamples=2, seed=5, return_sample=True)
        return m.refine_tokens(seq, DEV, draft, 1, cond_scale=2.0, timesteps=4, noise=NoiseSource(seed=41, sample0=5), return_sample=True)
    under_poison(arena, m, call)


def _switch_cases():
    from test_host_logic import FALLBACK_SWITCHES
    return [pytest.param(var, value, case, id=f"{var}={value}-{case}") for var, value, cases in FALLBACK_SWITCHES for case in cases]


@pytest.mark.parametrize("var,value,case", _switch_cases())
def test_every_fallback_switch_under_nan(var, value, case, arena, monkeypatch):
    """Each switch selects other kernels (tests/test_gpu_parity.py::test_every_fallback_switch_matches_reference): the program it
    selects, at B = 3, on an arena of NaNs against an arena of zeros."""
    monkeypatch.setenv(var, value)
    monkeypatch.setenv("MDT_F32_FUSED", "1")
    case, _, under = case.partition("+")
    if under:
        monkeypatch.setenv(*under.split("="))
    m = make_model(case)
    if var in ("MDT_B16", "MDT_QKV_MERGE", "MDT_RES16", "MDT_LNFOLD", "MDT_CAT_FOLD"):
        m.gemm_mode = "bf16"
    call = _sample(m, 8, 2.0) if var == "MDT_CFG_DUAL" else _denoise(m, 3, 1.0)      # (the dual / two-pass choice: under guidance only)
    outs = []
    for fill in (ZERO, NAN):
        arena.fill = fill
        _drop_arenas(m)
        before = arena.reallocations
        outs.append(call("X").clone())
        assert arena.reallocations > before and m._engine.handoff_status() == 0
    assert bool(torch.isfinite(outs[0]).all()) and torch.equal(_bits(outs[1]), _bits(outs[0]))


@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
def test_deep_unet_does_not_depend_on_what_reserve_allocated(mode, arena, monkeypatch):
    """BASELINE configs[4] architecture (512- and 1024-channel levels on the generic layer-by-layer kernels; in plain-bf16 mode the
    bf16 residual stream, PREP16 and the streamed bf16 GEMMs)."""
    monkeypatch.setenv("MDT_F32_FUSED", "1")
    m = make_model("cfg5")
    m.gemm_mode = mode
    under_poison(arena, m, _denoise(m, 3, 1.0))
