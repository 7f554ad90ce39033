"""-m gpu: the kernels of csrc/k_elem.hip against independent references at the shapes and edges where they can go wrong.

  generator     Philox4x32-10 + Box-Muller against the numpy transcription of the contract (noise_ref.py), with the high words of
                the key and the counter in use; every consumer's counter mode against its explicit mode, bit for bit
  flat kernels  one size past grid_for()'s cap of 2048 workgroups, so that the grid-stride loop takes a second trip
  tile kernels  the suite's arithmetic checks over edge shapes: L = 4, C == Cp, odd C, a Cp that is no power of two, L / 4 one
                past a wave, more samples than compute units, tiles above the 64 KiB default up to the 160 KiB ceiling
  dyn_scale     against a bit-level numpy reference of torch.quantile's interpolation (elem_ref.py): ties, padding, N = 4 .. 32768
  loss_rows     value against a float64 sum with a derived bound; the stated bitwise guarantees
  embeddings    mdt_cond_embed(_add) and MDT_OP_TIME_EMBED against float64 on the kernel's fp32 intermediates
  decode        first maximum, NaN wins: the five implementations against torch.argmax on NaN, signed zeros, ties and C = 1

Every measured figure is printed before it is asserted (`pytest -s`); DESIGN.md section 5 carries the measured values.
"""
import math

import numpy as np
import pytest
import torch

import elem_ref as R
import noise_ref
import test_gpu_samplers as S
from gpu_util import DEV, ref, rnd, run_both
from moleculediffusiontransformer_amd import runtime as rt
from moleculediffusiontransformer_amd.diffusion import scale_weights_rows

pytestmark = pytest.mark.gpu

TRIP = 2048 * 256           # work items of one trip of a flat kernel's grid-stride loop (grid_for()'s cap x the workgroup size)


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(got, want):
    """Bit-equal, any NaN standing for any NaN (the payload is not part of the contract)."""
    got, want = got.cpu(), want.cpu()
    nan = torch.isnan(want)
    return torch.equal(torch.isnan(got), nan) and torch.equal(bits(got)[~nan], bits(want)[~nan])


def xin_ok(xin, want_cl, C):
    """xin (B, L, Cp) token-major: the first C channels equal want (B, C, L) transposed bit for bit, the padding is exactly zero."""
    xin = xin.cpu()
    return torch.equal(xin[:, :, :C], want_cl.cpu().transpose(1, 2)) and bool((bits(xin[:, :, C:]) == 0).all())


def f32(v):
    return torch.tensor(v, dtype=torch.float32)


# ----------------------------------------------------------------------------------------------------------------------
# 3a. the generator against the host reference
# ----------------------------------------------------------------------------------------------------------------------
GEN_B, GEN_C, GEN_L, GEN_CP = 4, 16, 64, 16          # 256 quads per sample
KEYINGS = {                                           # (seed, draw, sample0)
    "plain": (1234, 3, 0),
    "high_seed_word": (0x9E3779B97F4A7C15, 3, 0),     # k1 = seed >> 32 != 0
    "largest_draw": (1234, 0xFFFFFFFF, 0),            # c2
    "straddle": (1234, 3, 2 ** 24 - 2),               # samples 0, 1: quad >> 32 == 0; samples 2, 3: == 1 (c1)
}
# Largest deviation of mdt_init_noise from noise_ref.normals measured on an MI355X (ROCm 7) over the four keyings: 3.4e-7.  The bound
# is 4x that, rounded up to one significant digit (device-library differences in logf / sincosf between ROCm versions), and may not
# exceed 1e-5: a conforming fp32 logf / sqrtf / sincosf at a few ulp on |z| <= 6.7 stays near 1e-6, any keying or ordering error is O(1).
NOISE_MEASURED = 3.356e-7
NOISE_TOL = 2e-6
assert 4 * NOISE_MEASURED <= NOISE_TOL <= 1e-5


def _draw(lib, st, key, B=GEN_B, C=GEN_C, L=GEN_L, draw=None):
    seed, d, s0 = key
    z = torch.empty(B, C, L, device=DEV)
    rt.check(lib.mdt_init_noise(rt.ptr(z), 0, 1.0, seed, d if draw is None else draw, s0, B, C, L, st))
    return z


@pytest.mark.parametrize("keying", list(KEYINGS))
def test_generator_matches_the_host_reference(keying):
    """mdt_init_noise(sigma0 = 1) against noise_ref.normals.  Measured max-abs deviation on an MI355X:
    plain 3.36e-7, high seed word 3.28e-7, largest draw 2.93e-7, straddle 3.01e-7; asserted at NOISE_TOL = 2e-6."""
    lib = rt.load_library()
    key = KEYINGS[keying]
    want = torch.from_numpy(noise_ref.normals(*key, GEN_B, GEN_C, GEN_L))
    with torch.cuda.device(DEV):
        st = rt.current_stream()
        z = _draw(lib, st, key)
        plain = _draw(lib, st, KEYINGS["plain"])
        torch.cuda.synchronize()
    dev = float((z.cpu().double() - want).abs().max())
    print(f"\nNOISE {keying} max|mdt_init_noise - host reference| = {dev:.3e}")
    assert dev <= NOISE_TOL, (keying, dev)
    if keying == "straddle":
        # the batch crosses the word boundary of the counter: the two halves differ, and neither is the stream of sample0 = 0
        assert (z[2:] - z[:2]).abs().max() > 1.0 and (z - plain).abs().max() > 1.0
        quad = (key[2] + torch.arange(GEN_B, dtype=torch.int64)) * (GEN_C * GEN_L // 4)
        assert [int(q) >> 32 for q in quad] == [0, 0, 1, 1]
    elif keying != "plain":
        assert (z - plain).abs().max() > 1.0


@pytest.mark.parametrize("keying", list(KEYINGS))
def test_every_consumer_of_the_generator_equals_its_explicit_mode(keying):
    """Counter mode == explicit mode fed with mdt_init_noise's tensor of the same (seed, draw, sample0), bit for bit."""
    lib = rt.load_library()
    seed, draw, s0 = key = KEYINGS[keying]
    B, C, L, Cp = GEN_B, GEN_C, GEN_L, GEN_CP
    x, xm, pred = rnd(B, C, L, seed=1) * 3, rnd(B, C, L, seed=2) * 3, rnd(B, L, Cp, seed=4)
    c_skip, c_out, c_in, sigma, sigma_mid, dt_down, up = 0.31, 0.095, 3.3, 0.29, 0.21, -0.11, 0.17
    gx, gxm, gp = (t.to(DEV).contiguous() for t in (x, xm, pred))
    mask = (rnd(B, C, L, seed=8) > 0).to(torch.uint8).to(DEV)
    gden = rnd(B, C, L, seed=5).to(DEV)
    w = scale_weights_rows(torch.tensor([9.0, 1.0, 0.3, 0.05]), 0.1)
    cf = w.packed().to(DEV)
    draw2 = draw ^ 1                                  # a second draw index for the re-noise of mdt_inpaint_enter
    with torch.cuda.device(DEV):
        st = rt.current_stream()
        z, z2 = _draw(lib, st, key), _draw(lib, st, key, draw=draw2)
        assert not torch.equal(z, z2)
        pairs = {}

        def both(name, call, *outs):
            """call(noise pointer, seed, draw, sample0) twice: counter mode, then the explicit tensor; outs are re-made per call."""
            got = []
            for noise, k in ((0, key), (rt.ptr(z), (0, 0, 0))):
                bufs = [o.clone() for o in outs]
                rt.check(call(noise, *k, *bufs))
                got.append(bufs)
            pairs[name] = got
            for a, b, o in zip(got[0], got[1], outs):
                assert torch.equal(bits(a), bits(b)), name
            assert not torch.equal(got[0][0], outs[0]), name          # the draw was applied

        both("add_noise", lambda n, sd, d, s, xa: lib.mdt_add_noise(rt.ptr(xa), n, 0.62, sd, d, s, B, C, L, st), gx)
        both("inpaint_merge", lambda n, sd, d, s, xa: lib.mdt_inpaint_merge(rt.ptr(xa), rt.ptr(gxm), rt.ptr(mask), n, 0.7, sd, d, s,
                                                                           B, C, L, st), gx)
        both("adpm2_euler", lambda n, sd, d, s, out: lib.mdt_adpm2_euler(rt.ptr(gx), rt.ptr(gxm), rt.ptr(gden), n,
                                                                         rt.ptr(out), sigma_mid, dt_down, up, 1 if n else 2, sd, d, s,
                                                                         B, C, L, st), torch.zeros_like(gx))
        xin = torch.full((B, L, Cp), 7.0, device=DEV)
        both("adpm2_next", lambda n, sd, d, s, xa, xi: lib.mdt_adpm2_next(rt.ptr(xa), rt.ptr(gxm), rt.ptr(gp), n, rt.ptr(xi), c_skip, c_out,
                                                                          sigma_mid, dt_down, up, c_in, sd, d, s, B, C, L, Cp, 0, 0, st),
             gx, xin)
        both("aeuler_next", lambda n, sd, d, s, xa, xi: lib.mdt_aeuler_next(rt.ptr(xa), rt.ptr(gp), n, rt.ptr(xi), c_skip, c_out, sigma,
                                                                            dt_down, up, c_in, sd, d, s, B, C, L, Cp, 0, 0, st), gx, xin)
        both("karras_hat", lambda n, sd, d, s, xh, xi: lib.mdt_karras_hat(rt.ptr(gx), n, rt.ptr(xh), rt.ptr(xi), 0.37, 1.003, c_in, sd, d, s,
                                                                          B, C, L, Cp, st), gx, xin)
        both("noise_in_rows", lambda n, sd, d, s, xn, xi: lib.mdt_noise_in_rows(rt.ptr(gx), n, rt.ptr(cf[0]), rt.ptr(cf[1]), rt.ptr(xn),
                                                                                rt.ptr(xi), sd, d, s, B, C, L, Cp, st), gx, xin)
        # mdt_inpaint_enter draws twice: the source's noise at `draw`, the re-noise at `draw2`, a mixed keep mask, renoise != 0
        got = []
        for ns, nr, k in ((0, 0, (seed, draw, draw2, s0)), (rt.ptr(z), rt.ptr(z2), (0, 0, 0, 0))):
            xa, xi = gx.clone(), xin.clone()
            rt.check(lib.mdt_inpaint_enter(rt.ptr(xa), rt.ptr(xi), rt.ptr(gxm), 0, rt.ptr(mask), 0, ns, nr, 2.75, 0.62, 0.36, *k,
                                           B, C, L, Cp, st))
            got.append((xa, xi))
        assert torch.equal(bits(got[0][0]), bits(got[1][0])) and torch.equal(bits(got[0][1]), bits(got[1][1]))
        m = mask.bool()
        assert torch.equal(got[0][0], torch.where(m, gxm + f32(2.75).to(DEV) * z, gx + f32(0.62).to(DEV) * z2))
        # the consumers see the reference's stream, not just each other's: one of them against the host reference
        torch.cuda.synchronize()
    # (2e-6: the fp32 roundings of 0.62, the product and the sum at |x| < 16)
    want = x.double() + 0.62 * torch.from_numpy(noise_ref.normals(*key, B, C, L))
    assert (pairs["add_noise"][0][0].cpu().double() - want).abs().max() <= 0.62 * NOISE_TOL + 2e-6


# ----------------------------------------------------------------------------------------------------------------------
# 3b. flat kernels past the grid cap
# ----------------------------------------------------------------------------------------------------------------------
FLAT = (130, 16, 1024)      # 2,129,920 elements = 532,480 float4s: the last 8,192 float4s are second-trip work


def _whole_and_tail(got, want, first_tail, what):
    got, want = got.cpu().reshape(-1), want.reshape(-1)
    assert got.numel() > first_tail
    assert torch.equal(bits(got[first_tail:]), bits(want[first_tail:])), f"{what}: the second trip of the grid-stride loop"
    assert torch.equal(bits(got), bits(want)), what


def test_flat_kernels_past_the_grid_cap():
    lib = rt.load_library()
    B, C, L = FLAT
    n = B * C * L
    assert n // 4 > TRIP
    x, xm, nz, den = rnd(B, C, L, seed=1) * 3, rnd(B, C, L, seed=2) * 3, rnd(B, C, L, seed=3), rnd(B, C, L, seed=4)
    cond, um = rnd(B, C, L, seed=5), rnd(B, C, L, seed=6)
    mask = rnd(B, C, L, seed=8) > 0
    gx, gxm, gnz, gden, gc, gu = (t.to(DEV) for t in (x, xm, nz, den, cond, um))
    gm = mask.to(torch.uint8).to(DEV)
    sigma, dt, up, T4 = 0.29, -0.11, 0.17, 4 * TRIP
    with torch.cuda.device(DEV):
        st = rt.current_stream()
        o = torch.empty_like(gx)
        rt.check(lib.mdt_init_noise(rt.ptr(o), rt.ptr(gnz), 2.5, 0, 0, 0, B, C, L, st))
        _whole_and_tail(o, f32(2.5) * nz, T4, "mdt_init_noise")
        o = gx.clone()
        rt.check(lib.mdt_add_noise(rt.ptr(o), rt.ptr(gnz), 0.62, 0, 0, 0, B, C, L, st))
        _whole_and_tail(o, x + f32(0.62) * nz, T4, "mdt_add_noise")
        euler = x + ((xm - den) / f32(sigma)) * f32(dt)
        for mode, want in ((0, euler), (1, euler + nz * f32(up))):
            o = torch.empty_like(gx)
            rt.check(lib.mdt_adpm2_euler(rt.ptr(gx), rt.ptr(gxm), rt.ptr(gden), rt.ptr(gnz), rt.ptr(o), sigma, dt, up, mode, 0, 0, 0,
                                         B, C, L, st))
            _whole_and_tail(o, want, T4, f"mdt_adpm2_euler mode {mode}")
        for sg, src in ((0.0, xm), (0.7, xm + f32(0.7) * nz)):
            o = gx.clone()
            rt.check(lib.mdt_inpaint_merge(rt.ptr(o), rt.ptr(gxm), rt.ptr(gm), rt.ptr(gnz), sg, 0, 0, 0, B, C, L, st))
            _whole_and_tail(o, torch.where(mask, src, x), T4, f"mdt_inpaint_merge sigma {sg}")
        o = gx.clone()
        rt.check(lib.mdt_clamp(rt.ptr(o), -1.0, 1.0, n, st))
        _whole_and_tail(o, x.clamp(-1, 1), T4, "mdt_clamp")
        o = torch.empty_like(gx)
        rt.check(lib.mdt_cfg_mix(rt.ptr(gc), rt.ptr(gu), rt.ptr(o), 7.5, n, st))
        _whole_and_tail(o, um + (cond - um) * 7.5, T4, "mdt_cfg_mix")
        # the counter mode takes the same loop: the tail of a long draw is the stream of its own global samples
        z = torch.empty_like(gx)
        rt.check(lib.mdt_init_noise(rt.ptr(z), 0, 1.0, 1234, 3, 0, B, C, L, st))
        torch.cuda.synchronize()
    want = torch.from_numpy(noise_ref.normals(1234, 3, 128, 2, C, L))
    assert (z[128:].cpu().double() - want).abs().max() <= NOISE_TOL


def test_concat_and_patch_past_the_grid_cap():
    A = rt.SP_ACT
    B, R_, Ca, Cb = 130, 64, 128, 128              # 8,320 rows x 64 float4s = 532,480 work items; samples 128, 129 are the second trip
    assert B * R_ * (Ca + Cb) // 4 > TRIP and 128 * R_ * (Ca + Cb) // 4 == TRIP
    act = torch.cat([rnd(B * R_ * Ca, seed=1), rnd(B * R_ * Cb, seed=2), torch.full((B * R_ * (Ca + Cb),), 7.0)])
    op = rt.MdtOp()
    op.kind = rt.OP_CONCAT
    op.a, op.a2, op.out = ref(A, 0), ref(A, R_ * Ca), ref(A, R_ * (Ca + Cb))
    op.i[rt.C_ROWS], op.i[rt.C_CA], op.i[rt.C_CB] = R_, Ca, Cb
    op.f[0] = 2 ** -0.5
    (ga, _, _), (ca, _, _) = run_both([op], torch.zeros(4), act, torch.zeros(4), {}, B)
    o0 = B * R_ * (Ca + Cb)
    _whole_and_tail(ga[o0:], ca[o0:], 128 * R_ * (Ca + Cb), "MDT_OP_CONCAT")
    a, b = act[: B * R_ * Ca].view(B * R_, Ca), act[B * R_ * Ca: o0].view(B * R_, Cb)
    assert torch.equal(ga[o0:].view(B * R_, Ca + Cb), torch.cat([a, b * f32(2 ** -0.5)], dim=1))
    # Patcher / Unpatcher round trip: one work item per element, 130 x 256 x 16 = 532,480
    L, C, p = 256, 16, 4
    assert B * L * C > TRIP and 128 * L * C == TRIP
    act = torch.cat([rnd(B * L * C, seed=3), torch.full((B * L * C,), 7.0), torch.full((B * L * C,), 7.0)])
    fwd, inv = rt.MdtOp(), rt.MdtOp()
    for o, (src, dst, inverse) in ((fwd, (0, L * C, 0)), (inv, (L * C, 2 * L * C, 1))):
        o.kind = rt.OP_PATCH
        o.a, o.out = ref(A, src), ref(A, dst)
        o.i[rt.P_ROWS_IN], o.i[rt.P_C_IN], o.i[rt.P_PATCH], o.i[rt.P_INVERSE] = L, C, p, inverse
        o.i[rt.P_LD_IN], o.i[rt.P_LD_OUT] = (C * p, C) if inverse else (C, C * p)
    (ga, _, _), (ca, _, _) = run_both([fwd, inv], torch.zeros(4), act, torch.zeros(4), {}, B)
    n = B * L * C
    x = act[:n].view(B, L, C).transpose(1, 2)
    y = x.reshape(B, C, L // p, p).permute(0, 1, 3, 2).reshape(B, C * p, L // p).transpose(1, 2).contiguous()
    _whole_and_tail(ga[n: 2 * n], y, 128 * L * C, "MDT_OP_PATCH forward")
    _whole_and_tail(ga[2 * n:], act[:n], 128 * L * C, "MDT_OP_PATCH inverse")
    assert torch.equal(ga, ca)


# ----------------------------------------------------------------------------------------------------------------------
# 3f. embeddings against float64
# ----------------------------------------------------------------------------------------------------------------------
def _cond_embed(lib, st, B, n, D1, D2, add):
    seq, w, b, freq = rnd(B, n, seed=11), rnd(D1, seed=12), rnd(D1, seed=13) * 0.5, R.inv_freq(D2)
    F = D1 if add else D1 + D2
    out = torch.full((B, n, F), 7.0, device=DEV)
    gs, gw, gb, gf = (t.to(DEV).contiguous() for t in (seq, w, b, freq))
    fn = lib.mdt_cond_embed_add if add else lib.mdt_cond_embed
    rt.check(fn(rt.ptr(gs), rt.ptr(gw), rt.ptr(gb), rt.ptr(gf), rt.ptr(out), B, n, D1, D2, st))
    torch.cuda.synchronize()
    return out.cpu().double(), R.cond_embed_ref(seq, w, b, freq, D2, add)


def _embed_close(got, want, what):
    """The project's bound for this kernel (test_additive_prelude_with_a_narrower_text_embedding): 1e-6 max(1, |value|)."""
    err = ((got - want).abs() / want.abs().clamp(min=1.0)).max()
    print(f"\nEMBED {what} max err / max(1, |v|) = {float(err):.3e}")
    assert float(err) < 1e-6, what


@pytest.mark.parametrize("B,n,D1,D2", [(1, 1, 16, 16), (3, 12, 32, 64), (2, 32, 64, 64), (5, 7, 24, 10)])
def test_cond_embed_against_fp64(B, n, D1, D2):
    lib = rt.load_library()
    with torch.cuda.device(DEV):
        got, want = _cond_embed(lib, rt.current_stream(), B, n, D1, D2, False)
    _embed_close(got, want, f"cond_embed {(B, n, D1, D2)}")


@pytest.mark.parametrize("B,n,D1,D2", [(2, 12, 32, 32), (2, 12, 8, 64), (3, 7, 24, 32)],
                         ids=["D1==D2", "only_sines", "sines_and_cosines"])
def test_cond_embed_add_against_fp64(B, n, D1, D2):
    lib = rt.load_library()
    with torch.cuda.device(DEV):
        got, want = _cond_embed(lib, rt.current_stream(), B, n, D1, D2, True)
    _embed_close(got, want, f"cond_embed_add {(B, n, D1, D2)}")


def test_cond_embed_past_the_grid_cap_and_refusals():
    lib = rt.load_library()
    B, n, D1, D2 = 130, 32, 64, 64                  # 532,480 work items; samples 128, 129 are the second trip
    assert B * n * (D1 + D2) > TRIP and 128 * n * (D1 + D2) == TRIP
    with torch.cuda.device(DEV):
        st = rt.current_stream()
        got, want = _cond_embed(lib, st, B, n, D1, D2, False)
        _embed_close(got[128:], want[128:], "cond_embed, the second trip of the grid-stride loop")
        _embed_close(got, want, "cond_embed past the grid cap")
        buf = torch.full((4096,), 7.0, device=DEV)
        p = rt.ptr(buf)
        assert lib.mdt_cond_embed(p, p, p, p, p, 2, 4, 8, 7, st) != 0            # D2 odd
        assert lib.mdt_cond_embed_add(p, p, p, p, p, 2, 4, 8, 7, st) != 0
        assert lib.mdt_cond_embed_add(p, p, p, p, p, 2, 4, 10, 8, st) != 0       # D1 > D2
        torch.cuda.synchronize()
        assert bool((buf == 7.0).all())


@pytest.mark.parametrize("n,half,ld", [(1, 1, 16), (7, 32, 80), (300, 16, 48)])
def test_time_embed_against_fp64(n, half, ld):
    W, S_ = rt.SP_WEIGHT, rt.SP_SHR
    off = (n + 15) // 16 * 16
    t = torch.linspace(-1.7, 0.55, n) if n > 1 else torch.tensor([0.37])
    shr = torch.cat([t, torch.zeros(off - n), torch.full((n * ld,), 7.0)])
    weights = rnd(half, seed=5)
    op = rt.MdtOp()
    op.kind = rt.OP_TIME_EMBED
    op.a, op.w, op.out = ref(S_, 0), ref(W, 0), ref(S_, off)
    op.i[rt.T_HALF], op.i[rt.T_LD] = half, ld
    (_, gs, _), _ = run_both([op], weights, torch.zeros(4), shr, {}, 1, n)
    got, want = gs[off:].view(n, ld), R.time_embed_ref(t, weights, ld)
    err = float((got.double() - want).abs().max())
    print(f"\nTIME_EMBED {(n, half, ld)} max err {err:.3e}")
    assert err < 2e-6
    assert torch.equal(got[:, 0], t) and bool((bits(got[:, 1 + 2 * half:]) == 0).all())
    assert torch.equal(gs[:off], shr[:off])


# ----------------------------------------------------------------------------------------------------------------------
# 3d. dynamic threshold against the bit-level reference
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,L,Cp", R.DYN_SHAPES)
def test_dyn_scale_equals_the_bit_level_reference(C, L, Cp):
    """mdt_dyn_scale and mdt_dyn_scale_rows == elem_ref.dyn_scale_ref exactly; within 2 ulp of torch.quantile (the reference stays
    within that on these inputs: tests/test_elem_ref_host.py)."""
    lib = rt.load_library()
    x, pred = R.dyn_inputs(C, L, Cp)
    gx, gp = x.to(DEV), pred.to(DEV)
    qs = R.DYN_QS + ([R.Q_INTEGRAL] if C * L == 2052 else [])
    rows_cs, rows_co = [c[0] for c in R.DYN_COEF], [c[1] for c in R.DYN_COEF]
    gcs, gco = f32(rows_cs).to(DEV), f32(rows_co).to(DEV)
    with torch.cuda.device(DEV):
        st = rt.current_stream()
        for q in qs:
            if q == R.Q_INTEGRAL:
                rank = np.float32(q) * np.float32(C * L - 1)
                assert rank == np.floor(rank) == np.float32(1000.0)
            for cs, co in R.DYN_COEF[:3]:
                ds = torch.full((4,), -1.0, device=DEV)
                rt.check(lib.mdt_dyn_scale(rt.ptr(gx), rt.ptr(gp), rt.ptr(ds), cs, co, q, 4, C, L, Cp, st))
                want = R.dyn_scale_ref(x, pred, cs, co, q)
                got = ds.cpu()
                assert torch.equal(bits(got), bits(want)), (q, cs, co, got, want)
                for b in range(4):
                    tq = max(torch.quantile(torch.from_numpy(R.magnitudes(x[b], pred[b], cs, co)), f32(q)).item(), 1.0)
                    assert abs(float(got[b]) - tq) <= 2 * float(np.spacing(np.float32(tq))), (q, cs, co, b)
            ds = torch.full((4,), -1.0, device=DEV)
            rt.check(lib.mdt_dyn_scale_rows(rt.ptr(gx), rt.ptr(gp), rt.ptr(ds), rt.ptr(gcs), rt.ptr(gco), q, 4, C, L, Cp, st))
            want = R.dyn_scale_ref(x, pred, rows_cs, rows_co, q)
            assert torch.equal(bits(ds.cpu()), bits(want)), (q, "rows", ds.cpu(), want)
            assert float(want[1]) == 1.0 and float(want[3]) == 2.5


def test_dyn_scale_refusals():
    lib = rt.load_library()
    C, L, Cp = 3, 10924, 16                          # C * L = 32772: one quad past the 32768 values the sort holds
    x, pred = torch.zeros(2, C, L, device=DEV), torch.zeros(2, L, Cp, device=DEV)
    ds, co = torch.full((2,), -1.0, device=DEV), torch.ones(2, device=DEV)
    with torch.cuda.device(DEV):
        st = rt.current_stream()
        for q, c, l in ((0.0, 3, 32), (1.5, 3, 32), (float("nan"), 3, 32), (0.9, C, L)):
            assert lib.mdt_dyn_scale(rt.ptr(x), rt.ptr(pred), rt.ptr(ds), 0.3, 0.1, q, 2, c, l, Cp, st) != 0, (q, c, l)
            assert lib.mdt_dyn_scale_rows(rt.ptr(x), rt.ptr(pred), rt.ptr(ds), rt.ptr(co), rt.ptr(co), q, 2, c, l, Cp, st) != 0, (q, c, l)
        torch.cuda.synchronize()
    assert bool((ds == -1.0).all())


# ----------------------------------------------------------------------------------------------------------------------
# 3c. tile kernels over edge shapes
# ----------------------------------------------------------------------------------------------------------------------
EDGE_SHAPES = [
    (1, 16, 4, 16),        # L = 4, no padding, C quads on 256 threads
    (3, 1, 4, 16),         # L = 4 with C = 1
    (2, 32, 32, 32),       # C == Cp above 16: tile_zero_pad with no padding columns
    (2, 33, 36, 48),       # odd C, Cp not a power of two, L / 4 = 9
    (2, 7, 260, 16),       # L / 4 = 65, one past a wave
    (257, 16, 8, 16),      # more workgroups than compute units
    (2, 16, 1024, 16),     # 68 KiB tile, above the 64 KiB default
    (2, 16, 2048, 16),     # 136 KiB tile; C L = 32768, the ceiling of mdt_dyn_scale and mdt_loss_rows
    (2, 3, 2408, 16),      # 163,744 B tile, the largest L at Cp = 16 that the ABI accepts
]
DYN_Q = 0.9


def _scale(lib, st, gx, gp, x, pred, c_skip, c_out, dims, dyn):
    """None, or the dynamic threshold's scale (B,) on the device -- the kernel's, after it has been found equal to the bit-level
    reference, which is what the expected values are formed with."""
    if not dyn:
        return None, None
    B, C, L, Cp = dims
    ds = torch.empty(B, device=DEV)
    rows = isinstance(c_skip, torch.Tensor)
    if rows:
        gcs, gco = c_skip.to(DEV), c_out.to(DEV)
        rt.check(lib.mdt_dyn_scale_rows(rt.ptr(gx), rt.ptr(gp), rt.ptr(ds), rt.ptr(gcs), rt.ptr(gco), DYN_Q, B, C, L, Cp, st))
        torch.cuda.synchronize()
        want = R.dyn_scale_ref(x, pred, c_skip.tolist(), c_out.tolist(), DYN_Q)
    else:
        rt.check(lib.mdt_dyn_scale(rt.ptr(gx), rt.ptr(gp), rt.ptr(ds), c_skip, c_out, DYN_Q, B, C, L, Cp, st))
        want = R.dyn_scale_ref(x, pred, c_skip, c_out, DYN_Q)
    assert torch.equal(bits(ds.cpu()), bits(want))
    return ds, want


def _same(got, want, dyn):
    if dyn:
        return float((got.cpu() - want).abs().max()) < S.DYN_TOL
    return torch.equal(bits(got.cpu()), bits(want))


@pytest.mark.parametrize("dyn", [False, True])
@pytest.mark.parametrize("dims", EDGE_SHAPES)
def test_precond_and_adpm2_kernels_over_edge_shapes(dims, dyn):
    lib = rt.load_library()
    B, C, L, Cp = dims
    x, xm, nz = rnd(B, C, L, seed=1) * 3, rnd(B, C, L, seed=2) * 3, rnd(B, C, L, seed=3)
    pred = rnd(B, L, Cp, seed=4)
    c_skip, c_out, c_in, sigma, sigma_mid, dt_mid, dt_down, up = 0.31, 0.095, 3.3, 0.29, 0.21, -0.08, -0.11, 0.17
    gx, gxm, gnz, gp = (t.to(DEV).contiguous() for t in (x, xm, nz, pred))
    p = pred[:, :, :C].transpose(1, 2)
    with torch.cuda.device(DEV):
        st = rt.current_stream()
        xin = torch.full((B, L, Cp), 7.0, device=DEV)
        rt.check(lib.mdt_precond_in(rt.ptr(gx), rt.ptr(xin), c_in, B, C, L, Cp, st))
        assert xin_ok(xin, f32(c_in) * x, C)
        ds, sc = _scale(lib, st, gx, gp, x, pred, c_skip, c_out, dims, dyn)
        den = S._clip(c_skip * x + c_out * p, sc)
        D = torch.empty_like(gx)
        rt.check(lib.mdt_precond_out(rt.ptr(gx), rt.ptr(gp), rt.ptr(D), c_skip, c_out, B, C, L, Cp, rt.ptr(ds), st))
        assert _same(D, den, dyn)
        out_mid, xin_mid = torch.empty_like(gx), torch.full((B, L, Cp), 7.0, device=DEV)
        rt.check(lib.mdt_adpm2_mid(rt.ptr(gx), rt.ptr(gp), rt.ptr(out_mid), rt.ptr(xin_mid), c_skip, c_out, sigma, dt_mid, c_in,
                                   B, C, L, Cp, rt.ptr(ds), st))
        x_mid = x + ((x - den) / f32(sigma)) * f32(dt_mid)
        assert _same(out_mid, x_mid, dyn)
        assert xin_ok(xin_mid, f32(c_in) * out_mid.cpu(), C)
        # second half, with xin_next ...
        ds2, sc2 = _scale(lib, st, gxm, gp, xm, pred, c_skip, c_out, dims, dyn)
        den2 = S._clip(c_skip * xm + c_out * p, sc2)
        want = x + ((xm - den2) / f32(sigma_mid)) * f32(dt_down)
        want = want + nz * f32(up)
        x2, xin2 = gx.clone(), torch.full((B, L, Cp), 7.0, device=DEV)
        rt.check(lib.mdt_adpm2_next(rt.ptr(x2), rt.ptr(gxm), rt.ptr(gp), rt.ptr(gnz), rt.ptr(xin2), c_skip, c_out, sigma_mid, dt_down, up,
                                    c_in, 0, 0, 0, B, C, L, Cp, 0, rt.ptr(ds2), st))
        assert _same(x2, want, dyn)
        assert xin_ok(xin2, f32(c_in) * x2.cpu(), C)
        # ... and as the last update of a call: the decode fused in
        x3, tok = gx.clone(), torch.full((B, L), -1, dtype=torch.int32, device=DEV)
        rt.check(lib.mdt_adpm2_next(rt.ptr(x3), rt.ptr(gxm), rt.ptr(gp), rt.ptr(gnz), 0, c_skip, c_out, sigma_mid, dt_down, up, 0.0,
                                    0, 0, 0, B, C, L, Cp, rt.ptr(tok), rt.ptr(ds2), st))
        assert torch.equal(bits(x3), bits(x2))
        assert torch.equal(tok.cpu().long(), x3.cpu().permute(0, 2, 1).argmax(dim=2))


@pytest.mark.parametrize("dyn", [False, True])
@pytest.mark.parametrize("dims", EDGE_SHAPES)
def test_aeuler_and_karras_kernels_over_edge_shapes(dims, dyn):
    """The bodies of test_gpu_samplers.py's kernel tests at the edge shapes; their dynamic scale (its `_dyn`) is the bit-level
    reference's, which the kernel's has to equal."""
    assert S.DYN_TOL == 1e-6
    S.test_aeuler_kernel_matches_reference_arithmetic(dims, dyn)
    S.test_karras_kernels_match_reference_arithmetic(dims, dyn)


@pytest.mark.parametrize("dims", EDGE_SHAPES)
def test_inpaint_enter_and_finish_over_edge_shapes(dims):
    lib = rt.load_library()
    B, C, L, Cp = dims
    x, src, n_src, n_re = (rnd(B, C, L, seed=s) for s in (31, 32, 33, 34))
    keep = rnd(B, C, L, seed=35) > 0
    keep[0, :, :4] = True                           # a quad with every element kept, and one with none
    keep[-1, :, -4:] = False
    sigma, renoise, c_in = 2.75, 0.62, 0.36
    gx, gs, gns, gnr = (t.to(DEV) for t in (x, src, n_src, n_re))
    gk = keep.to(torch.uint8).to(DEV)
    with torch.cuda.device(DEV):
        st = rt.current_stream()
        for rn in (0.0, renoise):
            want = torch.where(keep, src + f32(sigma) * n_src, x + f32(rn) * n_re if rn else x)
            xa, xin = gx.clone(), torch.full((B, L, Cp), 7.0, device=DEV)
            rt.check(lib.mdt_inpaint_enter(rt.ptr(xa), rt.ptr(xin), rt.ptr(gs), 0, rt.ptr(gk), 0, rt.ptr(gns), rt.ptr(gnr), sigma, rn, c_in,
                                           0, 0, 0, 0, B, C, L, Cp, st))
            assert torch.equal(bits(xa.cpu()), bits(want)), rn
            assert xin_ok(xin, f32(c_in) * want, C), rn
        # the exit: x = keep ? src : x, and the decode of the merged x
        xa, tok = gx.clone(), torch.full((B, L), -5, dtype=torch.int32, device=DEV)
        rt.check(lib.mdt_inpaint_finish(rt.ptr(xa), rt.ptr(gs), 0, rt.ptr(gk), 0, rt.ptr(tok), B, C, L, st))
        want = torch.where(keep, src, x)
        assert torch.equal(bits(xa.cpu()), bits(want))
        assert torch.equal(tok.cpu().long(), want.permute(0, 2, 1).argmax(dim=2))


def _row_sigmas(B):
    base = torch.tensor([9.0, 1.0, 0.3, 0.05, 0.001])
    return base.repeat((B + 4) // 5)[:B].clone()


@pytest.mark.parametrize("dyn", [False, True])
@pytest.mark.parametrize("dims", EDGE_SHAPES)
def test_per_sample_kernels_over_edge_shapes(dims, dyn):
    """mdt_noise_in_rows / mdt_precond_in_rows / mdt_precond_out_rows with B different coefficients, and mdt_loss_rows' value:
    the per-element term (clip(c_skip x + c_out pred) - x0)^2 formed in torch fp32 as the kernel forms it (bit-identical), summed
    in float64.  The kernel adds at most ceil(C L / 1024) * 4 terms per thread, 6 in the butterfly and 2 across the waves -- all
    non-negative -- and rounds the division and the weight: relative bound (ceil(C L / 1024) * 4 + 12) * 2^-24, derived, not tuned."""
    lib = rt.load_library()
    B, C, L, Cp = dims
    N = C * L
    x0, noise = rnd(B, C, L, seed=1, scale=0.5).clamp(-1, 1), rnd(B, C, L, seed=2)
    pred = rnd(B, L, Cp, seed=3) * 8               # c_out ~ 0.1 at the larger sigmas: the dynamic scale exceeds 1 there
    w = scale_weights_rows(_row_sigmas(B), 0.1)
    v = lambda t: t.view(-1, 1, 1)
    x_noisy = x0 + v(w.sigmas) * noise
    cf = w.packed().to(DEV).contiguous()
    gx0, gnz, gp = x0.to(DEV), noise.to(DEV), pred.to(DEV)
    p = pred[:, :, :C].transpose(1, 2)
    with torch.cuda.device(DEV):
        st = rt.current_stream()
        xn, xin = torch.empty(B, C, L, device=DEV), torch.full((B, L, Cp), 7.0, device=DEV)
        rt.check(lib.mdt_noise_in_rows(rt.ptr(gx0), rt.ptr(gnz), rt.ptr(cf[0]), rt.ptr(cf[1]), rt.ptr(xn), rt.ptr(xin), 0, 0, 0,
                                       B, C, L, Cp, st))
        assert torch.equal(bits(xn.cpu()), bits(x_noisy))
        assert xin_ok(xin, v(w.c_in) * x_noisy, C)
        xin2 = torch.full((B, L, Cp), 7.0, device=DEV)
        rt.check(lib.mdt_precond_in_rows(rt.ptr(xn), rt.ptr(xin2), rt.ptr(cf[1]), B, C, L, Cp, st))
        assert torch.equal(bits(xin2), bits(xin))
        ds, sc = _scale(lib, st, xn, gp, x_noisy, pred, w.c_skip, w.c_out, dims, dyn)
        assert sc is None or C * L < 16 or float(sc.max()) > 1.0
        den = S._clip(v(w.c_skip) * x_noisy + v(w.c_out) * p, sc)
        D = torch.empty_like(xn)
        rt.check(lib.mdt_precond_out_rows(rt.ptr(xn), rt.ptr(gp), rt.ptr(D), rt.ptr(cf[2]), rt.ptr(cf[3]), B, C, L, Cp, rt.ptr(ds), st))
        assert _same(D, den, dyn)
        loss = torch.full((B,), -1.0, device=DEV)
        rt.check(lib.mdt_loss_rows(rt.ptr(gx0), rt.ptr(xn), rt.ptr(gp), rt.ptr(cf[2]), rt.ptr(cf[3]), rt.ptr(cf[5]), rt.ptr(ds),
                                   rt.ptr(loss), B, C, L, Cp, st))
        torch.cuda.synchronize()
    r = den - x0
    want = (r * r).double().flatten(1).sum(1) / N * w.loss_weight.double()
    bound = (math.ceil(N / 1024) * 4 + 12) * 2.0 ** -24
    rel = float(((loss.cpu().double() - want).abs() / want).max())
    print(f"\nLOSS {dims} dyn={dyn} max rel err {rel:.3e} (bound {bound:.3e}) max scale {1.0 if sc is None else float(sc.max()):.3f}")
    assert rel <= bound, (dims, dyn, rel, bound)


def test_tile_kernels_refuse_what_the_abi_excludes():
    """Every entry point behind launch_tile's shape check: a tile above 160 KiB (L = 2412 at Cp = 16: 164,016 B), L % 4, Cp % 16, Cp < C --
    each returns non-zero and launches nothing (no buffer is touched)."""
    lib = rt.load_library()
    bad = [(2, 3, 2412, 16), (2, 3, 6, 16), (2, 3, 32, 24), (2, 20, 32, 16)]
    assert 2412 * 17 * 4 == 164016 > 160 * 1024 >= 2408 * 17 * 4
    n = 2 * 2412 * 32
    with torch.cuda.device(DEV):
        st = rt.current_stream()
        fb = [torch.full((n,), 7.0, device=DEV) for _ in range(6)]
        ib = torch.full((n,), 7, dtype=torch.int32, device=DEV)
        kb = torch.ones(n, dtype=torch.uint8, device=DEV)
        a, b, c, d, e, f = (rt.ptr(t) for t in fb)
        tk, kp = rt.ptr(ib), rt.ptr(kb)
        calls = {
            "mdt_precond_in": lambda *s: lib.mdt_precond_in(a, b, 3.3, *s, st),
            "mdt_precond_out": lambda *s: lib.mdt_precond_out(a, b, c, 0.3, 0.1, *s, 0, st),
            "mdt_noise_in_rows": lambda *s: lib.mdt_noise_in_rows(a, b, c, d, e, f, 0, 0, 0, *s, st),
            "mdt_precond_in_rows": lambda *s: lib.mdt_precond_in_rows(a, b, c, *s, st),
            "mdt_precond_out_rows": lambda *s: lib.mdt_precond_out_rows(a, b, c, d, e, *s, 0, st),
            "mdt_loss_rows": lambda *s: lib.mdt_loss_rows(a, b, c, d, e, f, 0, rt.ptr(fb[5][64:]), *s, st),
            "mdt_adpm2_mid": lambda *s: lib.mdt_adpm2_mid(a, b, c, d, 0.3, 0.1, 0.29, -0.08, 3.3, *s, 0, st),
            "mdt_adpm2_next": lambda *s: lib.mdt_adpm2_next(a, b, c, d, e, 0.3, 0.1, 0.21, -0.11, 0.17, 3.3, 0, 0, 0, *s, 0, 0, st),
            "mdt_aeuler_next": lambda *s: lib.mdt_aeuler_next(a, b, c, d, 0.3, 0.1, 0.29, -0.11, 0.17, 3.3, 0, 0, 0, *s, 0, 0, st),
            "mdt_aeuler_next (tokens)": lambda *s: lib.mdt_aeuler_next(a, b, c, 0, 0.3, 0.1, 0.29, -0.11, 0.17, 0.0, 0, 0, 0, *s, tk, 0, st),
            "mdt_karras_hat": lambda *s: lib.mdt_karras_hat(a, b, c, d, 0.37, 1.003, 3.3, 0, 0, 0, *s, st),
            "mdt_karras_mid": lambda *s: lib.mdt_karras_mid(a, b, c, d, e, 0.3, 0.1, 0.41, -0.12, 3.3, *s, 0, 0, st),
            "mdt_karras_next": lambda *s: lib.mdt_karras_next(a, b, c, d, e, 0.45, 0.08, 0.29, -0.06, *s, tk, 0, st),
            "mdt_inpaint_enter": lambda *s: lib.mdt_inpaint_enter(a, b, c, 0, kp, 0, d, e, 2.75, 0.62, 0.36, 0, 0, 0, 0, *s, st),
        }
        for name, call in calls.items():
            for shape in bad:
                assert call(*shape) != 0, (name, shape)
            assert "need L % 4 == 0" in lib.mdt_last_error().decode() and name.split()[0] in lib.mdt_last_error().decode()
        torch.cuda.synchronize()
        assert all(bool((t == 7.0).all()) for t in fb) and bool((ib == 7).all()), "a refused call wrote to a buffer"
        # the largest tile the ABI accepts is not refused (EDGE_SHAPES runs it); an empty batch is no error
        assert calls["mdt_precond_in"](0, 3, 2412, 16) == 0


# ----------------------------------------------------------------------------------------------------------------------
# 3e. mdt_loss_rows: the stated guarantees
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dyn", [False, True])
def test_loss_rows_is_bitwise_repeatable_and_position_independent(dyn):
    lib = rt.load_library()
    B, C, L, Cp = 5, 22, 32, 32
    x0, noise = rnd(B, C, L, seed=1, scale=0.5).clamp(-1, 1), rnd(B, C, L, seed=2)
    pred = rnd(B, L, Cp, seed=3) * 8
    w = scale_weights_rows(torch.tensor([9.0, 1.0, 0.3, 0.05, 0.001]), 0.1)
    x_noisy = x0 + w.sigmas.view(-1, 1, 1) * noise
    cf = w.packed()

    def run(idx):
        """The losses of samples idx, in that order, as one batch."""
        n = len(idx)
        g0, gn, gp, gc = (t[idx].contiguous().to(DEV) for t in (x0, x_noisy, pred, cf.t()))
        gc = gc.t().contiguous()
        ds = None
        if dyn:
            ds = torch.empty(n, device=DEV)
            rt.check(lib.mdt_dyn_scale_rows(rt.ptr(gn), rt.ptr(gp), rt.ptr(ds), rt.ptr(gc[2]), rt.ptr(gc[3]), DYN_Q, n, C, L, Cp, st))
            assert n < B or float(ds.max()) > 1.0
        loss = torch.full((n,), -1.0, device=DEV)
        rt.check(lib.mdt_loss_rows(rt.ptr(g0), rt.ptr(gn), rt.ptr(gp), rt.ptr(gc[2]), rt.ptr(gc[3]), rt.ptr(gc[5]), rt.ptr(ds),
                                   rt.ptr(loss), n, C, L, Cp, st))
        torch.cuda.synchronize()
        return loss.cpu()

    with torch.cuda.device(DEV):
        st = rt.current_stream()
        whole = run([0, 1, 2, 3, 4])
        assert bool((whole > 0).all()) and len(set(whole.tolist())) == B
        assert torch.equal(bits(run([0, 1, 2, 3, 4])), bits(whole)), "two calls"
        perm = [3, 0, 4, 1, 2]
        assert torch.equal(bits(run(perm)), bits(whole[perm])), "a permuted batch"
        for b in range(B):
            assert torch.equal(bits(run([b])), bits(whole[b: b + 1])), f"sample {b} alone"


# ----------------------------------------------------------------------------------------------------------------------
# 3g. decode semantics: first maximum, NaN wins, as torch.argmax -- all five implementations
# ----------------------------------------------------------------------------------------------------------------------
NAN, INF = float("nan"), float("inf")
DECODE_COLUMNS = [                   # (channel values, token)
    ([0.25, 0.25, 0.25, 0.25, 0.25], 0),          # an all-equal column
    ([-0.0, 0.0, -1.0, -1.0, -1.0], 0),           # -0.0 before +0.0: equal, the first wins
    ([0.0, -0.0, -1.0, -1.0, 0.0], 0),            # ... and the reverse
    ([0.25, NAN, 0.5, 0.9, 0.5], 1),              # one NaN, larger finite values after it
    ([0.25, NAN, 0.5, NAN, 0.9], 1),              # two NaNs: the first wins
    ([0.25, NAN, 0.5, INF, 0.5], 1),              # +inf after a NaN: the NaN wins
    ([0.25, 0.5, INF, 0.5, NAN], 4),              # a NaN after +inf wins too
    ([-1.0, 0.5, 0.9, 0.9, -0.5], 2),             # a plain tie
]


def _decode_target(C):
    """(2, C, 8): the columns above along l (C = 5), or a C = 1 tensor with the same special values (the token is always 0)."""
    cols = torch.tensor([c for c, _ in DECODE_COLUMNS], dtype=torch.float32)        # (8, 5)
    if C == 1:
        t = torch.stack([cols[:, 1], cols[:, 0]]).view(2, 1, 8)
        return t.contiguous(), torch.zeros(2, 8, dtype=torch.long)
    t = torch.stack([cols.t(), cols.t().flip(1)]).contiguous()
    tok = torch.tensor([k for _, k in DECODE_COLUMNS])
    return t, torch.stack([tok, tok.flip(0)])


@pytest.mark.parametrize("C", [5, 1])
def test_decode_semantics_of_all_five_implementations(C):
    lib = rt.load_library()
    target, tokens = _decode_target(C)
    B, _, L = target.shape
    Cp = 16
    want_tok = target.permute(0, 2, 1).argmax(dim=2)
    assert torch.equal(want_tok, tokens), "torch.argmax on the CPU: first maximum, NaN wins"
    assert C == 1 or (bool(torch.signbit(target[0, 0, 1])) and not bool(torch.signbit(target[0, 0, 2])))
    z0 = torch.where(target == 0, target, torch.zeros_like(target))      # the target's signed zeros, +0 elsewhere
    zeros = torch.zeros(B, L, Cp, device=DEV)
    gt, gz0 = target.to(DEV), z0.to(DEV)

    def check(name, x, tok):
        assert same_bits(x, target), f"{name}: the stored x"
        assert torch.equal(tok.cpu().long(), x.cpu().permute(0, 2, 1).argmax(dim=2)), f"{name}: tokens against argmax of the stored x"
        assert torch.equal(tok.cpu().long(), tokens), name

    with torch.cuda.device(DEV):
        st = rt.current_stream()
        new_tok = lambda: torch.full((B, L), -1, dtype=torch.int32, device=DEV)
        tok = new_tok()
        rt.check(lib.mdt_argmax_tokens(rt.ptr(gt), rt.ptr(tok), B, C, L, st))
        check("mdt_argmax_tokens", gt, tok)
        # mdt_inpaint_finish with nothing kept: x decides
        x, tok = gt.clone(), new_tok()
        keep = torch.zeros(B, C, L, dtype=torch.uint8, device=DEV)
        rt.check(lib.mdt_inpaint_finish(rt.ptr(x), rt.ptr(gz0), 0, rt.ptr(keep), 0, rt.ptr(tok), B, C, L, st))
        check("mdt_inpaint_finish", x, tok)
        # the fused decodes: the final x is steered to the target -- x = z0 (+ 0 * dt) + noise * 1 with noise = target, dt > 0 so
        # that a negative zero survives the sums
        x, tok = gz0.clone(), new_tok()
        rt.check(lib.mdt_adpm2_next(rt.ptr(x), rt.ptr(gz0), rt.ptr(zeros), rt.ptr(gt), 0, 0.31, 0.095, 0.21, 0.11, 1.0, 0.0, 0, 0, 0,
                                    B, C, L, Cp, rt.ptr(tok), 0, st))
        check("mdt_adpm2_next", x, tok)
        x, tok = gz0.clone(), new_tok()
        rt.check(lib.mdt_aeuler_next(rt.ptr(x), rt.ptr(zeros), rt.ptr(gt), 0, 0.31, 0.095, 0.29, 0.11, 1.0, 0.0, 0, 0, 0,
                                     B, C, L, Cp, rt.ptr(tok), 0, st))
        check("mdt_aeuler_next", x, tok)
        # no noise operand: the special values enter through x_hat; c_skip = 1, c_out = 0 and |finite| <= 1 make the denoised value
        # x_hat itself, so d = 0 and the Euler move returns x_hat
        d, x, tok = torch.empty_like(gt), torch.empty_like(gt), new_tok()
        rt.check(lib.mdt_karras_mid(rt.ptr(gt), rt.ptr(zeros), rt.ptr(d), rt.ptr(x), 0, 1.0, 0.0, 0.41, 0.12, 0.0, B, C, L, Cp,
                                    rt.ptr(tok), 0, st))
        check("mdt_karras_mid", x, tok)
        # the correction x = x_hat + half * (d + d') with d = x_next = z0: both derivatives are the target's signed zeros
        x, tok = torch.empty_like(gt), new_tok()
        rt.check(lib.mdt_karras_next(rt.ptr(gt), rt.ptr(gz0), rt.ptr(gz0), rt.ptr(zeros), rt.ptr(x), 0.45, 0.08, 0.29, 0.06, B, C, L, Cp,
                                     rt.ptr(tok), 0, st))
        check("mdt_karras_next", x, tok)
        torch.cuda.synchronize()
