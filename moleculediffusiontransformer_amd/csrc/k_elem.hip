// HBM-bound kernels of the sampling path on gfx950: k-diffusion preconditioning, the ADPM2 / AEuler / Karras sampler updates,
// noise generation, conditioning/time embeddings and the layout shuffles around the U-Net.
//
// Built with -ffp-contract=off: the sampler arithmetic keeps the reference's separate fp32 multiplies and
// adds (diffusion.py:417-435, :465-474, :502-515, :810-814) instead of fused multiply-adds.
//
// Sampler state, noise and results are (B, C, L) channel-major as in the reference; the U-Net consumes and
// produces token-major (B, L, Cp) tiles.  One workgroup handles one sample: the (L x Cp) tile is transposed
// through LDS so that both the channel-major and the token-major side are read and written as 16-byte
// coalesced accesses.  That pass exists once (tile_pass); an update kernel is its per-quad arithmetic on it,
// with one noise draw (draw4 / tile_draw) and one launcher (launch_tile) shared by all of them.  Two exceptions:
// k_inpaint_enter is left as it was, with its own loop, draws, source block and tail (measured slower in every
// shared form); the k_dyn_scale pair sorts a flat LDS array (dyn_scale_sample).  Both share only the launcher.
#include "mdt_kernels.h"
#include "../../include/mdt_hip.h"

namespace mdt {

// ------------------------------------------------------------------------------------------------
// Counter-based normal generator: Philox4x32-10 (Salmon et al., SC'11) + Box-Muller.
// One counter per 4 consecutive elements of the flattened GLOBAL (sample, channel, position) index, so
// the stream a sample sees does not depend on how the batch is sharded over GPUs.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1, uint32_t out[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    const uint32_t n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

__device__ __forceinline__ float4 normal4(uint64_t seed, uint32_t step, uint64_t quad_index) {
  uint32_t r[4];
  philox4x32_10((uint32_t)quad_index, (uint32_t)(quad_index >> 32), step, 0u, (uint32_t)seed,
                (uint32_t)(seed >> 32), r);
  const float k = 2.3283064365386963e-10f;  // 2^-32
  const float u0 = ((float)r[0] + 1.0f) * k, u1 = (float)r[1] * k;   // u0 in (0, 1]
  const float u2 = ((float)r[2] + 1.0f) * k, u3 = (float)r[3] * k;
  const float ra = sqrtf(-2.0f * logf(u0)), rb = sqrtf(-2.0f * logf(u2));
  float sa, ca, sb, cb;
  sincosf(6.283185307179586f * u1, &sa, &ca);
  sincosf(6.283185307179586f * u3, &sb, &cb);
  return make_float4(ra * ca, ra * sa, rb * cb, rb * sb);
}

__device__ __forceinline__ float clamp1(float v) { return fminf(fmaxf(v, -1.0f), 1.0f); }
// clip() of the denoised value (diffusion.py:75-88): static clamp to [-1, 1], or -- dynamic thresholding, s = the sample's
// max(quantile(|x_denoised|, q), 1) from k_dyn_scale -- clamp to [-s, s] and divide by s
__device__ __forceinline__ float clip_dyn(float v, float s) { return s > 0.f ? fminf(fmaxf(v, -s), s) / s : clamp1(v); }

// Token-major tile <-> LDS helpers (tile pitch Cp + 1 floats).
__device__ __forceinline__ void tile_load(float* tile, const float* src, int L, int Cp) {
  const int n4 = L * Cp / 4, c4n = Cp / 4;
  for (int i = threadIdx.x; i < n4; i += blockDim.x) {
    const float4 v = reinterpret_cast<const float4*>(src)[i];
    const int l = i / c4n, c = (i - l * c4n) * 4;
    float* t = tile + l * (Cp + 1) + c;
    t[0] = v.x; t[1] = v.y; t[2] = v.z; t[3] = v.w;
  }
}
__device__ __forceinline__ void tile_store(const float* tile, float* dst, int L, int Cp) {
  const int n4 = L * Cp / 4, c4n = Cp / 4;
  for (int i = threadIdx.x; i < n4; i += blockDim.x) {
    const int l = i / c4n, c = (i - l * c4n) * 4;
    const float* t = tile + l * (Cp + 1) + c;
    reinterpret_cast<float4*>(dst)[i] = make_float4(t[0], t[1], t[2], t[3]);
  }
}
__device__ __forceinline__ void tile_zero_pad(float* tile, int C, int L, int Cp) {
  const int np = Cp - C;
  for (int i = threadIdx.x; i < L * np; i += blockDim.x) {
    const int l = i / np, c = C + (i - l * np);
    tile[l * (Cp + 1) + c] = 0.f;
  }
}

// tokens[b,l] = argmax_c tile[l][c] (first maximum, NaN wins, as torch.argmax) of a tile that carries the final x
__device__ __forceinline__ void tile_argmax(const float* tile, int32_t* tokens, int b, int C, int L, int Cp) {
  for (int l = threadIdx.x; l < L; l += blockDim.x) {
    const float* t = tile + l * (Cp + 1);
    float best = t[0];
    int arg = 0;
    for (int c = 1; c < C; ++c) {
      const float v = t[c];
      if (v > best || (v != v && best == best)) { best = v; arg = c; }
    }
    tokens[(int64_t)b * L + l] = arg;
  }
}

// Four consecutive positions of one channel: what one thread moves per 16-byte access of a channel-major tensor.
struct Quad {
  float v[4];
  __device__ __forceinline__ float& operator[](int q) { return v[q]; }
  __device__ __forceinline__ float operator[](int q) const { return v[q]; }
};
__device__ __forceinline__ Quad load4(const float* p) {
  const float4 v = *reinterpret_cast<const float4*>(p);
  return {{v.x, v.y, v.z, v.w}};
}
__device__ __forceinline__ void store4(float* p, const Quad& a) { *reinterpret_cast<float4*>(p) = make_float4(a[0], a[1], a[2], a[3]); }

// A coefficient of the preconditioning: one for the batch, or one per sample (the *_rows kernels).
__device__ __forceinline__ float coef(float v, int) { return v; }
__device__ __forceinline__ float coef(const float* v, int b) { return v[b]; }

// The noise of quad i of a (B, C, L) tensor: the caller's tensor, or the counter-based generator at the GLOBAL quad index
// (elem0 = the flat index of the call's first element in the whole batch, a multiple of 4).
__device__ __forceinline__ float4 draw4(const float* noise, uint64_t seed, uint32_t step, int64_t elem0, int64_t i) {
  return noise ? reinterpret_cast<const float4*>(noise)[i] : normal4(seed, step, (uint64_t)((elem0 >> 2) + i));
}
// ... of the quad at element o of a tile kernel's shard, whose first sample is sample0 of the batch
__device__ __forceinline__ Quad tile_draw(const float* noise, uint64_t seed, uint32_t step, int64_t sample0, int C, int L, int64_t o) {
  const float4 nz = draw4(noise, seed, step, sample0 * C * L, o >> 2);
  return {{nz.x, nz.y, nz.z, nz.w}};
}

// The source of an inpaint / refine entry at channel c, positions ot .. ot + 3 of the flat (B, L) index: dense fp32 (B, C, L) at
// element o, or draft ids (B, L) standing for their +-1 one-hot (generative.py:1567-1569, :1603).
__device__ __forceinline__ Quad source4(const float* src, const int32_t* draft, int64_t o, int64_t ot, int c) {
  if (src) return load4(src + o);
  const int4 d4 = *reinterpret_cast<const int4*>(draft + ot);
  return {{c == d4.x ? 1.0f : -1.0f, c == d4.y ? 1.0f : -1.0f, c == d4.z ? 1.0f : -1.0f, c == d4.w ? 1.0f : -1.0f}};
}

// The scaffold of every "one workgroup per sample, one (L x Cp) tile in LDS" kernel.  A kernel is its per-quad arithmetic, a
// body(const TileQuad&) called once per (channel, four positions) of the sample, between
//   prologue: the U-Net's token-major output pred[b] staged in the tile (LoadPred) and the sample's dynamic-threshold scale;
//   tail:     xin != nullptr: the tile, zero-padded to Cp channels, stored token-major as the next network input;
//             else tokens != nullptr: the decode, tokens[b,l] = argmax_c tile[l][c]; else nothing.
// The body reads and writes channel-major tensors at p.o and the tile at p.t[q * p.pitch], q = 0..3 -- element (c, l + q) is
// touched by this one thread only, so the tile is reused in place (pred in, next input or final x out).
struct TileQuad {
  int b, c, l;     // sample (= workgroup), channel, first of the four positions
  int64_t o;       // flat (B, C, L) index of (b, c, l)
  float* t;        // tile element (l, c)
  int pitch;       // tile floats from position l to l + 1
  float ds;        // the sample's dynamic-threshold scale for clip_dyn, 0 = static clamp
};
template <bool LoadPred, class Body>
__device__ __forceinline__ void tile_pass(float* tile, const float* pred, const float* dscale, float* xin, int32_t* tokens,
                                          int C, int L, int Cp, Body body) {
  const int b = blockIdx.x;
  const float ds = dscale ? dscale[b] : 0.f;
  if (LoadPred) { tile_load(tile, pred + (int64_t)b * L * Cp, L, Cp); __syncthreads(); }
  const int l4n = L / 4;
  for (int e = threadIdx.x; e < C * l4n; e += blockDim.x) {
    const int c = e / l4n, l = (e - c * l4n) * 4;
    body(TileQuad{b, c, l, (int64_t)b * C * L + c * L + l, tile + l * (Cp + 1) + c, Cp + 1, ds});
  }
  // (a kernel whose xin is not optional stores nothing for a null xin, where its own tail would have faulted)
  if (xin) { tile_zero_pad(tile, C, L, Cp); __syncthreads(); tile_store(tile, xin + (int64_t)b * L * Cp, L, Cp); }
  else if (tokens) { __syncthreads(); tile_argmax(tile, tokens, b, C, L, Cp); }
}

// xin[b,l,c] = c_in * x[b,c,l]                                             (diffusion.py:810)
template <class Coef>
__device__ __forceinline__ void precond_in(float* tile, const float* x, float* xin, Coef c_in, int C, int L, int Cp) {
  const float ci = coef(c_in, blockIdx.x);
  tile_pass<false>(tile, nullptr, nullptr, xin, nullptr, C, L, Cp, [=](const TileQuad& p) {
    const Quad xv = load4(x + p.o);
#pragma unroll
    for (int q = 0; q < 4; ++q) p.t[q * p.pitch] = ci * xv[q];
  });
}
__global__ __launch_bounds__(256) void k_precond_in(const float* x, float* xin, float c_in, int C, int L, int Cp) {
  extern __shared__ float tile[];
  precond_in(tile, x, xin, c_in, C, L, Cp);
}

// D = clamp(c_skip*x + c_out*pred, -1, 1)                                  (diffusion.py:811-814)
template <class Coef>
__device__ __forceinline__ void precond_out(float* tile, const float* x, const float* pred, float* D, Coef c_skip, Coef c_out,
                                            int C, int L, int Cp, const float* dscale) {
  const float cs = coef(c_skip, blockIdx.x), co = coef(c_out, blockIdx.x);
  tile_pass<true>(tile, pred, dscale, nullptr, nullptr, C, L, Cp, [=](const TileQuad& p) {
    const Quad xv = load4(x + p.o);
    Quad d;
#pragma unroll
    for (int q = 0; q < 4; ++q) d[q] = clip_dyn(cs * xv[q] + co * p.t[q * p.pitch], p.ds);
    store4(D + p.o, d);
  });
}
__global__ __launch_bounds__(256) void k_precond_out(const float* x, const float* pred, float* D, float c_skip,
                                                      float c_out, int C, int L, int Cp, const float* dscale) {
  extern __shared__ float tile[];
  precond_out(tile, x, pred, D, c_skip, c_out, C, L, Cp, dscale);
}

// Dynamic thresholding (clip() with dynamic_threshold = q > 0, diffusion.py:78-88): per sample
//   scale[b] = max(torch.quantile(|c_skip x + c_out pred|.flatten(), q), 1)
// One workgroup per sample: the N = C L magnitudes are sorted in LDS (bitonic, padded with +inf to a power of two) and the
// quantile is torch's linear interpolation between the two neighbouring order statistics: rank = q (N - 1) in fp32,
// lerp(v[floor], v[ceil], rank - floor) with ATen's two-sided formula.  The consumers (k_precond_out / k_adpm2_mid / k_adpm2_next)
// then clamp to [-scale, scale] and divide.  Rarely used (every class of the reference passes 0.0): simple, not tuned.
__device__ __forceinline__ void dyn_scale_sample(float* tile, const float* x, const float* pred, float* scale, float c_skip,
                                                 float c_out, float q, int C, int L, int Cp, int npad) {
  const int b = blockIdx.x, N = C * L;
  const float* xb = x + (int64_t)b * N;
  const float* pb = pred + (int64_t)b * L * Cp;
  for (int e = threadIdx.x; e < npad; e += blockDim.x) {
    float v = INFINITY;
    if (e < N) {
      const int c = e / L, l = e - c * L;
      v = fabsf(c_skip * xb[e] + c_out * pb[l * Cp + c]);
    }
    tile[e] = v;
  }
  __syncthreads();
  for (int k = 2; k <= npad; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int e = threadIdx.x; e < npad; e += blockDim.x) {
        const int p = e ^ j;
        if (p > e) {
          const float a0 = tile[e], a1 = tile[p];
          const bool up = (e & k) == 0;
          if ((a0 > a1) == up) { tile[e] = a1; tile[p] = a0; }
        }
      }
      __syncthreads();
    }
  if (threadIdx.x == 0) {
    const float rank = q * (float)(N - 1);
    const float below = floorf(rank), above = ceilf(rank);
    const float w = rank - below;
    const float v0 = tile[(int)below], v1 = tile[(int)above];
    const float diff = v1 - v0;
    const float qv = fabsf(w) < 0.5f ? v0 + w * diff : v1 - diff * (1.0f - w);
    scale[b] = fmaxf(qv, 1.0f);
  }
}
__global__ __launch_bounds__(256) void k_dyn_scale(const float* x, const float* pred, float* scale, float c_skip, float c_out,
                                                    float q, int C, int L, int Cp, int npad) {
  extern __shared__ float tile[];
  dyn_scale_sample(tile, x, pred, scale, c_skip, c_out, q, C, L, Cp, npad);
}
// ... with one (c_skip, c_out) pair per sample (KDiffusion_mod.forward: one sigma per sample, diffusion.py:820-844)
__global__ __launch_bounds__(256) void k_dyn_scale_rows(const float* x, const float* pred, float* scale, const float* c_skip,
                                                         const float* c_out, float q, int C, int L, int Cp, int npad) {
  extern __shared__ float tile[];
  dyn_scale_sample(tile, x, pred, scale, c_skip[blockIdx.x], c_out[blockIdx.x], q, C, L, Cp, npad);
}

// First half of ADPM2Sampler.step fused with denoise_fn's output stage   (diffusion.py:506-508, :811-814)
__global__ __launch_bounds__(256) void k_adpm2_mid(const float* x, const float* pred, float* x_mid, float* xin_mid,
                                                    float c_skip, float c_out, float sigma, float dt_mid,
                                                    float c_in_mid, int C, int L, int Cp, const float* dscale) {
  extern __shared__ float tile[];
  tile_pass<true>(tile, pred, dscale, xin_mid, nullptr, C, L, Cp, [=](const TileQuad& p) {
    const Quad xv = load4(x + p.o);
    Quad xm;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float* t = p.t + q * p.pitch;
      const float den = clip_dyn(c_skip * xv[q] + c_out * (*t), p.ds);
      const float d = (xv[q] - den) / sigma;
      xm[q] = xv[q] + d * dt_mid;
      *t = c_in_mid * xm[q];   // same thread owns (l, c): in-place reuse of the tile for xin_mid
    }
    store4(x_mid + p.o, xm);
  });
}

// Second half of ADPM2Sampler.step                                        (diffusion.py:510-515)
// tokens != nullptr (last step of a call): also the decode step after the path, tokens[b,l] = argmax_c x[b,c,l] of the
// final x (generative.py:1212-1213, :1690-1691: permute(0,2,1) -> argmax(dim=2); first maximum, NaN wins, as torch.argmax),
// taken from the values this kernel has in LDS anyway instead of a second pass over the (B, C, L) result.
__global__ __launch_bounds__(256) void k_adpm2_next(float* x, const float* x_mid, const float* pred,
                                                     const float* noise, float* xin_next, float c_skip, float c_out,
                                                     float sigma_mid, float dt_down, float sigma_up, float c_in_next,
                                                     uint64_t seed, uint32_t step, int64_t sample0, int C, int L,
                                                     int Cp, int32_t* tokens, const float* dscale) {
  extern __shared__ float tile[];
  const bool keep_x = tokens && !xin_next;       // the tile then carries x itself (not c_in_next * x) for the argmax
  tile_pass<true>(tile, pred, dscale, xin_next, tokens, C, L, Cp, [=](const TileQuad& p) {
    const Quad xv = load4(x + p.o), mv = load4(x_mid + p.o), nv = tile_draw(noise, seed, step, sample0, C, L, p.o);
    Quad xn;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float* t = p.t + q * p.pitch;
      const float den = clip_dyn(c_skip * mv[q] + c_out * (*t), p.ds);
      const float d = (mv[q] - den) / sigma_mid;
      float xx = xv[q] + d * dt_down;
      xx = xx + nv[q] * sigma_up;
      xn[q] = xx;
      *t = keep_x ? xx : c_in_next * xx;
    }
    store4(x + p.o, xn);
  });
}

// The whole AEulerSampler.step after its one evaluation                   (diffusion.py:465-474, :811-814)
//   den = clip(c_skip x + c_out pred); d = (x - den) / sigma; x' = x + d * dt; x' = x' + noise * sigma_up
// k_adpm2_next without the x_mid stream: the derivative is taken at x itself.  xin_next / tokens as there.
__global__ __launch_bounds__(256) void k_aeuler_next(float* x, const float* pred, const float* noise, float* xin_next,
                                                      float c_skip, float c_out, float sigma, float dt, float sigma_up,
                                                      float c_in_next, uint64_t seed, uint32_t step, int64_t sample0,
                                                      int C, int L, int Cp, int32_t* tokens, const float* dscale) {
  extern __shared__ float tile[];
  const bool keep_x = tokens && !xin_next;       // the tile then carries x itself (not c_in_next * x) for the argmax
  tile_pass<true>(tile, pred, dscale, xin_next, tokens, C, L, Cp, [=](const TileQuad& p) {
    const Quad xv = load4(x + p.o), nv = tile_draw(noise, seed, step, sample0, C, L, p.o);
    Quad xn;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float* t = p.t + q * p.pitch;
      const float den = clip_dyn(c_skip * xv[q] + c_out * (*t), p.ds);
      const float d = (xv[q] - den) / sigma;
      float xx = xv[q] + d * dt;
      xx = xx + nv[q] * sigma_up;
      xn[q] = xx;
      *t = keep_x ? xx : c_in_next * xx;
    }
    store4(x + p.o, xn);
  });
}

// KarrasSampler.step, the churn stage                                      (diffusion.py:424-425, :810)
//   x_hat = x + ns * (s_noise * noise), ns = fp32(sqrt(sigma_hat^2 - sigma^2));   xin = c_in_hat * x_hat
// x_hat may be x (every element is read and written by one thread).
__global__ __launch_bounds__(256) void k_karras_hat(const float* x, const float* noise, float* x_hat, float* xin, float ns,
                                                     float s_noise, float c_in_hat, uint64_t seed, uint32_t step,
                                                     int64_t sample0, int C, int L, int Cp) {
  extern __shared__ float tile[];
  tile_pass<false>(tile, nullptr, nullptr, xin, nullptr, C, L, Cp, [=](const TileQuad& p) {
    const Quad xv = load4(x + p.o), nv = tile_draw(noise, seed, step, sample0, C, L, p.o);
    Quad xh;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float eps = s_noise * nv[q];
      xh[q] = xv[q] + ns * eps;
      p.t[q * p.pitch] = c_in_hat * xh[q];
    }
    store4(x_hat + p.o, xh);
  });
}

// KarrasSampler.step, the Euler move from sigma_hat to sigma_next          (diffusion.py:427-429, :811-814)
//   den = clip(c_skip x_hat + c_out pred); d = (x_hat - den) / sigma_hat; x_next = x_hat + dt * d
// d is kept for the correction; xin_next = c_in_next * x_next for the second evaluation, or (sigma_next == 0: no
// correction, x_next is the step's result) NULL, then with the optional fused decode of k_adpm2_next.
__global__ __launch_bounds__(256) void k_karras_mid(const float* x_hat, const float* pred, float* d_out, float* x_next,
                                                     float* xin_next, float c_skip, float c_out, float sigma_hat, float dt,
                                                     float c_in_next, int C, int L, int Cp, int32_t* tokens,
                                                     const float* dscale) {
  extern __shared__ float tile[];
  tile_pass<true>(tile, pred, dscale, xin_next, tokens, C, L, Cp, [=](const TileQuad& p) {
    const Quad xv = load4(x_hat + p.o);
    Quad dv, xn;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float* t = p.t + q * p.pitch;
      const float den = clip_dyn(c_skip * xv[q] + c_out * (*t), p.ds);
      dv[q] = (xv[q] - den) / sigma_hat;
      xn[q] = xv[q] + dt * dv[q];
      *t = xin_next ? c_in_next * xn[q] : xn[q];
    }
    store4(d_out + p.o, dv);
    store4(x_next + p.o, xn);
  });
}

// KarrasSampler.step, the second-order correction AS THE REFERENCE WRITES IT (diffusion.py:432-434, :811-814)
//   den = clip(c_skip x_next + c_out pred); d' = (x_next - den) / sigma_next; x = x_hat + half * (d + d'),
//   half = 0.5 * (sigma - sigma_hat)        (zero without churn: the step then returns x_hat)
// x may be x_hat (one thread per element).  tokens != nullptr: the fused decode of the final x.
__global__ __launch_bounds__(256) void k_karras_next(const float* x_hat, const float* x_next, const float* d_in,
                                                      const float* pred, float* x, float c_skip, float c_out,
                                                      float sigma_next, float half, int C, int L, int Cp, int32_t* tokens,
                                                      const float* dscale) {
  extern __shared__ float tile[];
  tile_pass<true>(tile, pred, dscale, nullptr, tokens, C, L, Cp, [=](const TileQuad& p) {
    const Quad hv = load4(x_hat + p.o), mv = load4(x_next + p.o), dv = load4(d_in + p.o);
    Quad xn;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float* t = p.t + q * p.pitch;
      const float den = clip_dyn(c_skip * mv[q] + c_out * (*t), p.ds);
      const float dp = (mv[q] - den) / sigma_next;
      xn[q] = hv[q] + half * (dv[q] + dp);
      *t = xn[q];
    }
    store4(x + p.o, xn);
  });
}

// Flat (B*C*L) kernels: 4 elements per thread.
__global__ __launch_bounds__(256) void k_init_noise(float* x, const float* noise, float sigma0, uint64_t seed,
                                                     uint32_t step, int64_t elem0, int64_t n4) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 nz = draw4(noise, seed, step, elem0, i);
    reinterpret_cast<float4*>(x)[i] = make_float4(sigma0 * nz.x, sigma0 * nz.y, sigma0 * nz.z, sigma0 * nz.w);
  }
}

__global__ __launch_bounds__(256) void k_add_noise(float* x, const float* noise, float s, uint64_t seed, uint32_t step,
                                                    int64_t elem0, int64_t n4) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 nz = draw4(noise, seed, step, elem0, i);
    float4 v = reinterpret_cast<float4*>(x)[i];
    v.x = v.x + s * nz.x; v.y = v.y + s * nz.y; v.z = v.z + s * nz.z; v.w = v.w + s * nz.w;
    reinterpret_cast<float4*>(x)[i] = v;
  }
}

// One Euler move of ADPM2Sampler.step with the denoised tensor supplied by the caller's fn (diffusion.py:506-515):
//   out = x_base + ((x_from - den) / sigma) * dt   [+ noise * sigma_up]
// first half: x_base = x_from = x, dt = sigma_mid - sigma; second half: x_base = x, x_from = x_mid, dt = sigma_down - sigma
__global__ __launch_bounds__(256) void k_adpm2_euler(const float* xb, const float* xf, const float* den, const float* noise,
                                                      float* out, float sigma, float dt, float sigma_up, int noise_mode,
                                                      uint64_t seed, uint32_t step, int64_t elem0, int64_t n4) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 b = reinterpret_cast<const float4*>(xb)[i], f = reinterpret_cast<const float4*>(xf)[i];
    const float4 d = reinterpret_cast<const float4*>(den)[i];
    float4 o;
    o.x = b.x + ((f.x - d.x) / sigma) * dt; o.y = b.y + ((f.y - d.y) / sigma) * dt;
    o.z = b.z + ((f.z - d.z) / sigma) * dt; o.w = b.w + ((f.w - d.w) / sigma) * dt;
    if (noise_mode) {
      const float4 nz = draw4(noise_mode == 1 ? noise : nullptr, seed, step, elem0, i);   // mode 2: the generator
      o.x = o.x + nz.x * sigma_up; o.y = o.y + nz.y * sigma_up; o.z = o.z + nz.z * sigma_up; o.w = o.w + nz.w * sigma_up;
    }
    reinterpret_cast<float4*>(out)[i] = o;
  }
}

// x = where(mask, src + sigma*noise, x)                                    (diffusion.py:539-542, :549)
__global__ __launch_bounds__(256) void k_inpaint_merge(float* x, const float* src, const uint8_t* mask,
                                                        const float* noise, float sigma, uint64_t seed, uint32_t step,
                                                        int64_t elem0, int64_t n4) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    float4 nz = make_float4(0.f, 0.f, 0.f, 0.f);
    if (sigma != 0.0f) nz = draw4(noise, seed, step, elem0, i);
    const float4 sv = reinterpret_cast<const float4*>(src)[i];
    const uchar4 mk = reinterpret_cast<const uchar4*>(mask)[i];
    float4 v = reinterpret_cast<float4*>(x)[i];
    if (sigma != 0.0f) {
      if (mk.x) v.x = sv.x + sigma * nz.x;
      if (mk.y) v.y = sv.y + sigma * nz.y;
      if (mk.z) v.z = sv.z + sigma * nz.z;
      if (mk.w) v.w = sv.w + sigma * nz.w;
    } else {
      if (mk.x) v.x = sv.x;
      if (mk.y) v.y = sv.y;
      if (mk.z) v.z = sv.z;
      if (mk.w) v.w = sv.w;
    }
    reinterpret_cast<float4*>(x)[i] = v;
  }
}

// The entry of one inpainting resample (diffusion.py:539-547, :810) in one pass: k_add_noise (re-noise of the previous resample,
// skipped when renoise == 0), k_inpaint_merge and k_precond_in, op for op, on one read of x:
//   x = keep ? src + sigma * n_src : x + renoise * n_re;   xin = c_in * x (token-major, padded)
// src: dense fp32 (B, C, L), or draft ids (B, L) standing for their +-1 one-hot (generative.py:1567-1569, :1603).  keep: uint8
// (B, C, L), or (B, L) broadcast over channels (keep_tok).  n_src / n_re == nullptr: the counter-based generator at draw index
// step_src / step_re and the GLOBAL element index, as the flat kernels.  One workgroup per sample, as k_precond_in.
// Left as it was, on neither tile_pass nor the shared helpers: as a tile_pass body, with its own loop on tile_draw and source4, and
// with its own loop and draws on source4 alone, it gave the same bits from the same registers but ran 7 - 8 % slower alone, far
// outside the spread of repeats (profiles/tile_pass_ab.txt); the cause was not found.  Its quad index and its source block are
// second copies of tile_draw's and source4's: a change to either is made here too.
__global__ __launch_bounds__(256) void k_inpaint_enter(float* x, float* xin, const float* src, const int32_t* draft,
                                                        const uint8_t* keep, int keep_tok, const float* n_src,
                                                        const float* n_re, float sigma, float renoise, float c_in,
                                                        uint64_t seed, uint32_t step_src, uint32_t step_re, int64_t sample0,
                                                        int C, int L, int Cp) {
  extern __shared__ float tile[];
  const int b = blockIdx.x;
  const int l4n = L / 4;
  for (int e = threadIdx.x; e < C * l4n; e += blockDim.x) {
    const int c = e / l4n, l = (e - c * l4n) * 4;
    const int64_t o = (int64_t)b * C * L + c * L + l, ot = (int64_t)b * L + l;
    const uint64_t quad = (uint64_t)(((sample0 + b) * C + c) * (int64_t)L + l) >> 2;
    const uchar4 mk = *reinterpret_cast<const uchar4*>(keep + (keep_tok ? ot : o));
    const bool kv[4] = {mk.x != 0, mk.y != 0, mk.z != 0, mk.w != 0};
    const bool any = kv[0] || kv[1] || kv[2] || kv[3], all = kv[0] && kv[1] && kv[2] && kv[3];
    const float4 v = *reinterpret_cast<const float4*>(x + o);
    float xn[4] = {v.x, v.y, v.z, v.w};
    if (renoise != 0.0f && !all) {                       // (a kept element's re-noised value is overwritten by the merge)
      const float4 nz = n_re ? *reinterpret_cast<const float4*>(n_re + o) : normal4(seed, step_re, quad);
      const float nv[4] = {nz.x, nz.y, nz.z, nz.w};
#pragma unroll
      for (int q = 0; q < 4; ++q) xn[q] = xn[q] + renoise * nv[q];
    }
    if (any) {
      float sv[4];
      if (src) {
        const float4 s4 = *reinterpret_cast<const float4*>(src + o);
        sv[0] = s4.x; sv[1] = s4.y; sv[2] = s4.z; sv[3] = s4.w;
      } else {
        const int4 d4 = *reinterpret_cast<const int4*>(draft + ot);
        sv[0] = c == d4.x ? 1.0f : -1.0f; sv[1] = c == d4.y ? 1.0f : -1.0f;
        sv[2] = c == d4.z ? 1.0f : -1.0f; sv[3] = c == d4.w ? 1.0f : -1.0f;
      }
      if (sigma != 0.0f) {
        const float4 nz = n_src ? *reinterpret_cast<const float4*>(n_src + o) : normal4(seed, step_src, quad);
        const float nv[4] = {nz.x, nz.y, nz.z, nz.w};
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (kv[q]) xn[q] = sv[q] + sigma * nv[q];
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (kv[q]) xn[q] = sv[q];
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) tile[(l + q) * (Cp + 1) + c] = c_in * xn[q];
    *reinterpret_cast<float4*>(x + o) = make_float4(xn[0], xn[1], xn[2], xn[3]);
  }
  tile_zero_pad(tile, C, L, Cp);
  __syncthreads();
  tile_store(tile, xin + (int64_t)b * L * Cp, L, Cp);
}

// The entry of a refine call (the expression of diffusion.py:535, then :810): the rows whose start step is the loop's current
// step i get their noised source as state and its scaled copy as network input,
//   start[b] == i:  x = src + sigma * n;   xin = c_in * x (token-major, padded)
// and every other workgroup returns at once, writing neither x nor xin: a row that has not started yet rides along with its
// state ignored, a row that has started keeps what the update kernels left.  src / draft, n == nullptr and the quad index as
// k_inpaint_enter.  One workgroup per sample.
__global__ __launch_bounds__(256) void k_refine_enter(float* x, float* xin, const int32_t* start, int step_i, const float* src,
                                                       const int32_t* draft, const float* noise, float sigma, float c_in,
                                                       uint64_t seed, uint32_t step, int64_t sample0, int C, int L, int Cp) {
  extern __shared__ float tile[];
  if (start[blockIdx.x] != step_i) return;               // (uniform over the workgroup, before any barrier: none is skipped by a part of it)
  tile_pass<false>(tile, nullptr, nullptr, xin, nullptr, C, L, Cp, [=](const TileQuad& p) {
    const Quad sv = source4(src, draft, p.o, (int64_t)p.b * L + p.l, p.c);
    const Quad nv = tile_draw(noise, seed, step, sample0, C, L, p.o);
    Quad xn;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      xn[q] = sv[q] + sigma * nv[q];
      p.t[q * p.pitch] = c_in * xn[q];
    }
    store4(x + p.o, xn);
  });
}

// The per-step entry of a refine call around a kept scaffold: k_refine_enter's entry and the merge of ADPM2Sampler.inpaint
// (diffusion.py:539-542, as a select) in front of step i, then :810, on one read of the state:
//   start[b] >  i:  nothing -- the workgroup returns at once, writing neither x nor xin;
//   start[b] == i:  x = keep ? src + sigma * n_src : src + sigma * n_entry;
//   start[b] <  i:  x = keep ? src + sigma * n_src : x;
// and for the rows that run xin = c_in * x (token-major, padded).  A quad takes only the draws it needs: a fully kept quad no
// entry draw, a started quad with nothing kept none (nor its source, nor a store of x).  src / draft as k_refine_enter, keep /
// keep_tok as k_inpaint_enter; n_entry / n_src == nullptr: the generator at draw index step_entry / step_src.  One workgroup
// per sample.
__global__ __launch_bounds__(256) void k_refine_keep_enter(float* x, float* xin, const int32_t* start, int step_i, const float* src,
                                                            const int32_t* draft, const uint8_t* keep, int keep_tok,
                                                            const float* n_entry, const float* n_src, float sigma, float c_in,
                                                            uint64_t seed, uint32_t step_entry, uint32_t step_src, int64_t sample0,
                                                            int C, int L, int Cp) {
  extern __shared__ float tile[];
  const int s0 = start[blockIdx.x];
  if (s0 > step_i) return;                               // (uniform over the workgroup, before any barrier: none is skipped by a part of it)
  const bool entering = s0 == step_i;
  tile_pass<false>(tile, nullptr, nullptr, xin, nullptr, C, L, Cp, [=](const TileQuad& p) {
    const int64_t ot = (int64_t)p.b * L + p.l;
    const uchar4 mk = *reinterpret_cast<const uchar4*>(keep + (keep_tok ? ot : p.o));
    const bool kv[4] = {mk.x != 0, mk.y != 0, mk.z != 0, mk.w != 0};
    const bool any = kv[0] || kv[1] || kv[2] || kv[3], all = kv[0] && kv[1] && kv[2] && kv[3];
    Quad xn = {{0.f, 0.f, 0.f, 0.f}};
    if (!entering) xn = load4(x + p.o);
    if (entering || any) {
      const Quad sv = source4(src, draft, p.o, ot, p.c);
      if (entering && !all) {                            // (a kept element's entry value is overwritten by the merge)
        const Quad nv = tile_draw(n_entry, seed, step_entry, sample0, C, L, p.o);
#pragma unroll
        for (int q = 0; q < 4; ++q) xn[q] = sv[q] + sigma * nv[q];
      }
      if (any) {
        const Quad nv = tile_draw(n_src, seed, step_src, sample0, C, L, p.o);
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (kv[q]) xn[q] = sv[q] + sigma * nv[q];
      }
      store4(x + p.o, xn);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) p.t[q * p.pitch] = c_in * xn[q];
  });
}

// The last merge of ADPM2Sampler.inpaint (diffusion.py:549: sigma 0) and the decode (generative.py:1613-1614), one thread per
// position: x = keep ? src : x; tokens[b,l] = argmax_c x[b,c,l] (first maximum, as k_argmax) -- with draft ids and a per-position
// keep, a kept position's token is its draft id.  src / draft / keep / keep_tok as k_inpaint_enter; tokens may be nullptr.
__global__ __launch_bounds__(256) void k_inpaint_finish(float* x, const float* src, const int32_t* draft, const uint8_t* keep,
                                                         int keep_tok, int32_t* tokens, int B, int C, int L) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= (int64_t)B * L) return;
  const int b = (int)(i / L), l = (int)(i - (int64_t)b * L);
  const int d = draft ? draft[i] : -1;
  const bool kt = keep_tok && keep[i] != 0;
  float* p = x + (int64_t)b * C * L + l;
  float best = 0.f;
  int arg = 0;
  for (int c = 0; c < C; ++c) {
    const int64_t o = (int64_t)c * L;
    float v = p[o];
    if (keep_tok ? kt : keep[(int64_t)b * C * L + l + o] != 0) {
      v = src ? src[(int64_t)b * C * L + l + o] : (c == d ? 1.0f : -1.0f);
      p[o] = v;
    }
    if (c == 0 || v > best || (v != v && best == best)) { best = v; arg = c; }
  }
  if (tokens) tokens[i] = (draft && kt) ? d : arg;
}

// dst[0..n) = src[0..n): the FiLM rows of ONE evaluation out of the table the time program fills once per call.  One small launch on
// the caller's stream (hipMemcpyAsync of the same bytes ran as up to three runtime copy kernels of ~4 us each in front of every
// evaluation graph: profiles/r6_kernel_stats.csv, __amd_rocclr_copyBuffer).
__global__ __launch_bounds__(256) void k_copy_f32(float* __restrict__ dst, const float* __restrict__ src, int64_t n, int vec) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (vec) {
    if (t < n / 4) reinterpret_cast<float4*>(dst)[t] = reinterpret_cast<const float4*>(src)[t];
  } else {
    for (int64_t k = t; k < n; k += (int64_t)gridDim.x * 256) dst[k] = src[k];
  }
}

__global__ __launch_bounds__(256) void k_clamp(float* x, float lo, float hi, int64_t n4) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    float4 v = reinterpret_cast<float4*>(x)[i];
    v.x = fminf(fmaxf(v.x, lo), hi); v.y = fminf(fmaxf(v.y, lo), hi);
    v.z = fminf(fmaxf(v.z, lo), hi); v.w = fminf(fmaxf(v.w, lo), hi);
    reinterpret_cast<float4*>(x)[i] = v;
  }
}

// out = um + (cond - um) * scale                                           (modules.py:1253)
__global__ __launch_bounds__(256) void k_cfg_mix(const float* cond, const float* um, float* out, float scale,
                                                  int64_t n4) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 c = reinterpret_cast<const float4*>(cond)[i], u = reinterpret_cast<const float4*>(um)[i];
    reinterpret_cast<float4*>(out)[i] = make_float4(u.x + (c.x - u.x) * scale, u.y + (c.y - u.y) * scale,
                                                    u.z + (c.z - u.z) * scale, u.w + (c.w - u.w) * scale);
  }
}

// k_cfg_mix with one scale per sample: out[b] = scale[b] == 1 ? cond[b] : um[b] + (cond[b] - um[b]) * scale[b].  A row of row4
// float4s is cut into segments of G float4s (G a power of two <= 256: the lanes of one segment); a workgroup holds 256 / G
// segments per trip of the grid-stride loop over the B * segs segments.  A segment reads its sample's scale once; at scale 1 the
// reference skips guidance (modules.py:1248) -- um is not read, and u + (c - u) would not be c in fp32.
__global__ __launch_bounds__(256) void k_cfg_mix_rows(const float* cond, const float* um, float* out, const float* scale,
                                                       int64_t row4, int64_t segs, int64_t units, int G) {
  const int per_wg = 256 / G, lane = threadIdx.x & (G - 1);
  for (int64_t u = blockIdx.x * (int64_t)per_wg + threadIdx.x / G; u < units; u += (int64_t)gridDim.x * per_wg) {
    const int64_t b = u / segs, i = (u - b * segs) * G + lane;
    if (i >= row4) continue;
    const float s = scale[b];
    const int64_t o = b * row4 + i;
    const float4 c = reinterpret_cast<const float4*>(cond)[o];
    if (s == 1.0f) {
      reinterpret_cast<float4*>(out)[o] = c;
    } else {
      const float4 v = reinterpret_cast<const float4*>(um)[o];
      reinterpret_cast<float4*>(out)[o] = make_float4(v.x + (c.x - v.x) * s, v.y + (c.y - v.y) * s, v.z + (c.z - v.z) * s,
                                                      v.w + (c.w - v.w) * s);
    }
  }
}

// tokens[b,l] = argmax_c x[b,c,l] (first maximum, as torch.argmax)          (generative.py:1212-1213)
__global__ __launch_bounds__(256) void k_argmax(const float* x, int32_t* tok, int B, int C, int L) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= (int64_t)B * L) return;
  const int b = (int)(i / L), l = (int)(i - (int64_t)b * L);
  const float* p = x + (int64_t)b * C * L + l;
  float best = p[0];
  int arg = 0;
  for (int c = 1; c < C; ++c) {
    const float v = p[(int64_t)c * L];
    if (v > best || (v != v && best == best)) { best = v; arg = c; }
  }
  tok[i] = arg;
}

// e[b,i,:D1] = gelu(w*s+b), e[b,i,D1:] = [sin(i f) | cos(i f)]             (generative.py:838-850, transformer.py:3456-3470)
// add != 0 (pos_emb_fourier_add, generative.py:844-846): e[b,i,f] = gelu(w*s+b)[f] + PositionalEncoding1D(D2)[i,f], f < D1 <= D2
// (the reference's encoding returns emb[:, :, :orig_ch], the FIRST D1 columns of [sin (D2/2) | cos (D2/2)], transformer.py:3470)
__global__ __launch_bounds__(256) void k_cond_embed(const float* seq, const float* w, const float* bias,
                                                     const float* inv_freq, float* out, int B, int n, int D1, int D2, int add) {
  const int F = add ? D1 : D1 + D2;
  const int64_t total = (int64_t)B * n * F;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int f = (int)(i % F);
    const int64_t row = i / F;
    const int pos = (int)(row % n);
    float v = 0.f;
    if (f < D1) {
      const float h = seq[row] * w[f] + bias[f];
      v = 0.5f * h * (1.0f + erff(h * 0.70710678118654752440f));
    }
    if (add || f >= D1) {
      const int j = add ? f : f - D1, half = D2 / 2;
      const float arg = (float)pos * inv_freq[j < half ? j : j - half];
      const float pe = j < half ? sinf(arg) : cosf(arg);
      v = add ? v + pe : pe;
    }
    out[i] = v;
  }
}

// LearnedPositionalEmbedding: [t, sin(t w 2 pi), cos(t w 2 pi)] padded to ld  (modules.py:554-559)
__global__ __launch_bounds__(256) void k_time_embed(const float* cn, const float* w, float* out, int rows, int half,
                                                     int ld) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * ld) return;
  const int r = i / ld, c = i - r * ld;
  const float t = cn[r];
  float v = 0.f;
  if (c == 0) v = t;
  else if (c <= 2 * half) {
    const int j = c - 1;
    const float fr = t * w[j < half ? j : j - half] * 2.0f * 3.14159265358979323846f;
    v = j < half ? sinf(fr) : cosf(fr);
  }
  out[i] = v;
}

// out[row, :ca] = a[row, :], out[row, ca:ca+cb] = b[row, :] * scale_b       (modules.py:828-829)
__global__ __launch_bounds__(256) void k_concat(const float* a, const float* b, float* out, int64_t rows, int ca,
                                                 int cb, float scale_b) {
  const int w4 = (ca + cb) / 4, ca4 = ca / 4;
  const int64_t total = rows * w4;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = i / w4;
    const int c = (int)(i - row * w4);
    float4 v;
    if (c < ca4) v = reinterpret_cast<const float4*>(a)[row * ca4 + c];
    else {
      v = reinterpret_cast<const float4*>(b)[row * (cb / 4) + (c - ca4)];
      v.x *= scale_b; v.y *= scale_b; v.z *= scale_b; v.w *= scale_b;
    }
    reinterpret_cast<float4*>(out)[i] = v;
  }
}

// Patcher 'b c (l p) -> b (c p) l' / Unpatcher ' b (c p) l -> b c (l p) ' on token-major tensors
// (modules.py:230, :255): fwd  y[b, l, c*p + q] = x[b, l*p + q, c];  inverse the other way round.
__global__ __launch_bounds__(256) void k_patch(const float* in, float* out, int batch, int rows_in, int c_in, int ld_in,
                                                int ld_out, int patch, int inverse) {
  // rows_in / c_in always describe the UNPATCHED side (long sequence, few channels).
  const int64_t total = (int64_t)batch * rows_in * c_in;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % c_in);
    const int64_t t = i / c_in;
    const int r = (int)(t % rows_in);
    const int64_t b = t / rows_in;
    const int l = r / patch, q = r - l * patch;
    const int64_t long_idx = (b * rows_in + r) * (int64_t)(inverse ? ld_out : ld_in) + c;
    const int64_t short_idx = (b * (rows_in / patch) + l) * (int64_t)(inverse ? ld_in : ld_out) + c * patch + q;
    if (inverse) out[long_idx] = in[short_idx];
    else out[short_idx] = in[long_idx];
  }
}

// ------------------------------------------------------------------------------------------------
// One noise level PER SAMPLE (KDiffusion_mod.forward / denoise_fn(sigmas=(B,)), diffusion.py:798-844): the kernels above with
// their coefficients read from device vectors of B entries, and the training objective's value as one fused pass.
// ------------------------------------------------------------------------------------------------
// x_noisy = x0 + sigma[b] * noise (diffusion.py:828-829), xin = c_in[b] * x_noisy (:810).  noise == nullptr: the counter-based
// generator keyed by (seed, step, global sample index), as k_init_noise.
__global__ __launch_bounds__(256) void k_noise_in_rows(const float* x0, const float* noise, const float* sigma, const float* c_in,
                                                        float* x_noisy, float* xin, uint64_t seed, uint32_t step, int64_t sample0,
                                                        int C, int L, int Cp) {
  extern __shared__ float tile[];
  const float sg = sigma[blockIdx.x], ci = c_in[blockIdx.x];
  tile_pass<false>(tile, nullptr, nullptr, xin, nullptr, C, L, Cp, [=](const TileQuad& p) {
    const Quad xv = load4(x0 + p.o), nv = tile_draw(noise, seed, step, sample0, C, L, p.o);
    Quad xn;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      xn[q] = xv[q] + sg * nv[q];
      p.t[q * p.pitch] = ci * xn[q];
    }
    store4(x_noisy + p.o, xn);
  });
}

// xin[b,l,c] = c_in[b] * x[b,c,l]
__global__ __launch_bounds__(256) void k_precond_in_rows(const float* x, float* xin, const float* c_in, int C, int L, int Cp) {
  extern __shared__ float tile[];
  precond_in(tile, x, xin, c_in, C, L, Cp);
}

// D = clip(c_skip[b] * x + c_out[b] * pred)
__global__ __launch_bounds__(256) void k_precond_out_rows(const float* x, const float* pred, float* D, const float* c_skip,
                                                           const float* c_out, int C, int L, int Cp, const float* dscale) {
  extern __shared__ float tile[];
  precond_out(tile, x, pred, D, c_skip, c_out, C, L, Cp, dscale);
}

// loss[b] = weight[b] * mean_{c,l} ((clip(c_skip[b] x_noisy + c_out[b] pred) - x0)^2)   (diffusion.py:838-844), the denoised
// tensor never written.  The sum runs in a fixed order: every thread over its own elements in ascending order, the 64 lanes of a
// wave by a butterfly, the four waves' partials as (w0 + w1) + (w2 + w3) -- two calls give the same bits, and a sample's value
// does not depend on its position in the batch.
__global__ __launch_bounds__(256) void k_loss_rows(const float* x0, const float* x_noisy, const float* pred, const float* c_skip,
                                                    const float* c_out, const float* weight, const float* dscale, float* loss,
                                                    int C, int L, int Cp) {
  extern __shared__ float tile[];
  float* red = tile;                                 // the waves' partial sums reuse the tile once every thread is done with it
  const int b = blockIdx.x;
  const float cs = c_skip[b], co = c_out[b];
  float acc = 0.f;
  tile_pass<true>(tile, pred, dscale, nullptr, nullptr, C, L, Cp, [=, &acc](const TileQuad& p) {
    const Quad xv = load4(x_noisy + p.o), tv = load4(x0 + p.o);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float den = clip_dyn(cs * xv[q] + co * p.t[q * p.pitch], p.ds);
      const float r = den - tv[q];
      acc = acc + r * r;
    }
  });
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) loss[b] = weight[b] * (((red[0] + red[1]) + (red[2] + red[3])) / (float)(C * L));
}

static inline unsigned grid_for(int64_t n, int block = 256, int cap = 256 * 8) {
  int64_t g = (n + block - 1) / block;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (unsigned)g;
}

hipError_t launch_concat(const float* a, const float* b, float* out, int64_t rows, int ca, int cb, float scale_b,
                         hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_concat, dim3(grid_for(rows * (ca + cb) / 4)), dim3(256), 0, s, a, b, out, rows, ca, cb, scale_b);
  return hipGetLastError();
}
hipError_t launch_patch(const float* in, float* out, int batch, int rows_in, int c_in, int ld_in, int ld_out, int patch,
                        int inverse, hipStream_t s) {
  if (batch <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_patch, dim3(grid_for((int64_t)batch * rows_in * c_in)), dim3(256), 0, s, in, out, batch,
                     rows_in, c_in, ld_in, ld_out, patch, inverse);
  return hipGetLastError();
}
hipError_t launch_time_embed(const float* cn, const float* w, float* out, int rows, int half, int ld, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_time_embed, dim3((rows * ld + 255) / 256), dim3(256), 0, s, cn, w, out, rows, half, ld);
  return hipGetLastError();
}

}  // namespace mdt

// ------------------------------------------------------------------------------------------------
// C ABI entry points of this translation unit (declared in include/mdt_hip.h)
// ------------------------------------------------------------------------------------------------
namespace {
inline size_t tile_bytes(int L, int Cp) { return (size_t)L * (Cp + 1) * sizeof(float); }

// Launch of a kernel that holds one sample in dynamic LDS, one workgroup of 256 per sample: up to the CU's 160 KiB (the default limit
// of a launch is 64 KiB: raised once per kernel and device -- per device, not per process, mdt_kernels.h).
constexpr size_t kMaxLds = 160 * 1024;
template <auto Kernel, class... A>
int launch_lds(const char* name, int B, size_t lds, void* stream, A... args) {
  static mdt::DevOnce once;
  if (once.first()) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds);
  hipLaunchKernelGGL(Kernel, dim3(B), dim3(256), lds, (hipStream_t)stream, args...);
  return mdt_finish(name);
}
// The entry of every tile kernel: an empty batch is no error, the tile's shape is checked (max_length = 1024, the reference
// constructors' default, at 16 padded channels is 68 KiB), then `refuse` -- what this entry point excludes beyond that, or nullptr.
template <auto Kernel, class... A>
int launch_tile(const char* name, const char* refuse, int B, int C, int L, int Cp, void* stream, A... args) {
  if (B <= 0) return 0;
  if (L % 4 || Cp % 16 || Cp < C) return mdt_bad(name, ": need L % 4 == 0, Cp % 16 == 0, Cp >= C");
  if (tile_bytes(L, Cp) > kMaxLds) return mdt_bad(name, ": (L, Cp) tile exceeds the 160 KiB of LDS of a compute unit");
  if (refuse) return mdt_bad(name, refuse);
  return launch_lds<Kernel>(name, B, tile_bytes(L, Cp), stream, args...);
}
// mdt_dyn_scale / mdt_dyn_scale_rows: the coefficients as float or as const float* per sample; `refuse` as launch_tile's
template <auto Kernel, class Coef>
int launch_dyn_scale(const char* name, const char* refuse, const float* x, const float* pred, float* scale, Coef c_skip, Coef c_out, float q,
                     int B, int C, int L, int Cp, void* stream) {
  if (B <= 0) return 0;
  if (refuse) return mdt_bad(name, refuse);
  if (!(q > 0.0f && q <= 1.0f)) return mdt_bad(name, ": the quantile must lie in (0, 1]");
  if (C <= 0 || L <= 0 || Cp < C) return mdt_bad(name, ": bad dims");
  int npad = 1;
  while (npad < C * L) npad <<= 1;
  if ((size_t)npad * sizeof(float) > kMaxLds) return mdt_bad(name, ": C * L exceeds 32768 values (the sort runs in one compute unit's LDS)");
  return launch_lds<Kernel>(name, B, (size_t)npad * sizeof(float), stream, x, pred, scale, c_skip, c_out, q, C, L, Cp, npad);
}
}  // namespace

extern "C" {

int mdt_cond_embed(const float* seq, const float* fc1_w, const float* fc1_b, const float* inv_freq, float* out,
                   int32_t B, int32_t n, int32_t D1, int32_t D2, void* stream) {
  if (B <= 0) return 0;
  if (D2 % 2) return mdt_bad("mdt_cond_embed: D2 must be even");
  hipLaunchKernelGGL(mdt::k_cond_embed, dim3(mdt::grid_for((int64_t)B * n * (D1 + D2))), dim3(256), 0,
                     (hipStream_t)stream, seq, fc1_w, fc1_b, inv_freq, out, B, n, D1, D2, 0);
  return mdt_finish("mdt_cond_embed");
}

int mdt_cond_embed_add(const float* seq, const float* fc1_w, const float* fc1_b, const float* inv_freq, float* out,
                       int32_t B, int32_t n, int32_t D1, int32_t D2, void* stream) {
  if (!seq || !fc1_w || !fc1_b || !inv_freq || !out) return mdt_bad("mdt_cond_embed_add: null pointer");
  if (B <= 0) return 0;
  if (D1 <= 0 || D2 <= 0 || D2 % 2 || D1 > D2) return mdt_bad("mdt_cond_embed_add: need 0 < D1 <= D2, D2 even");
  hipLaunchKernelGGL(mdt::k_cond_embed, dim3(mdt::grid_for((int64_t)B * n * D1)), dim3(256), 0, (hipStream_t)stream, seq,
                     fc1_w, fc1_b, inv_freq, out, B, n, D1, D2, 1);
  return mdt_finish("mdt_cond_embed_add");
}

int mdt_precond_in(const float* x, float* xin, float c_in, int32_t B, int32_t C, int32_t L, int32_t Cp,
                   void* stream) {
  return launch_tile<mdt::k_precond_in>("mdt_precond_in", nullptr, B, C, L, Cp, stream, x, xin, c_in, C, L, Cp);
}

int mdt_precond_out(const float* x, const float* pred, float* D, float c_skip, float c_out, int32_t B, int32_t C,
                    int32_t L, int32_t Cp, const float* dyn_scale, void* stream) {
  return launch_tile<mdt::k_precond_out>("mdt_precond_out", nullptr, B, C, L, Cp, stream, x, pred, D, c_skip, c_out, C, L, Cp,
                                         dyn_scale);
}

int mdt_dyn_scale(const float* x, const float* pred, float* scale, float c_skip, float c_out, float q, int32_t B, int32_t C,
                  int32_t L, int32_t Cp, void* stream) {
  const char* refuse = !x || !pred || !scale ? ": null pointer" : nullptr;
  return launch_dyn_scale<mdt::k_dyn_scale>("mdt_dyn_scale", refuse, x, pred, scale, c_skip, c_out, q, B, C, L, Cp, stream);
}

/* ---- one noise level per sample (include/mdt_hip.h: "per-sample noise levels") ---- */
int mdt_noise_in_rows(const float* x0, const float* noise, const float* sigma, const float* c_in, float* x_noisy, float* xin,
                      uint64_t seed, uint32_t step, int64_t sample0, int32_t B, int32_t C, int32_t L, int32_t Cp, void* stream) {
  const char* refuse = !x0 || !sigma || !c_in || !x_noisy || !xin ? ": null pointer" : nullptr;
  return launch_tile<mdt::k_noise_in_rows>("mdt_noise_in_rows", refuse, B, C, L, Cp, stream, x0, noise, sigma, c_in, x_noisy, xin,
                                           seed, step, sample0, C, L, Cp);
}

int mdt_precond_in_rows(const float* x, float* xin, const float* c_in, int32_t B, int32_t C, int32_t L, int32_t Cp, void* stream) {
  const char* refuse = !x || !xin || !c_in ? ": null pointer" : nullptr;
  return launch_tile<mdt::k_precond_in_rows>("mdt_precond_in_rows", refuse, B, C, L, Cp, stream, x, xin, c_in, C, L, Cp);
}

int mdt_precond_out_rows(const float* x, const float* pred, float* D, const float* c_skip, const float* c_out, int32_t B, int32_t C,
                         int32_t L, int32_t Cp, const float* dyn_scale, void* stream) {
  const char* refuse = !x || !pred || !D || !c_skip || !c_out ? ": null pointer" : nullptr;
  return launch_tile<mdt::k_precond_out_rows>("mdt_precond_out_rows", refuse, B, C, L, Cp, stream, x, pred, D, c_skip, c_out, C, L,
                                              Cp, dyn_scale);
}

int mdt_dyn_scale_rows(const float* x, const float* pred, float* scale, const float* c_skip, const float* c_out, float q, int32_t B,
                       int32_t C, int32_t L, int32_t Cp, void* stream) {
  const char* refuse = !x || !pred || !scale || !c_skip || !c_out ? ": null pointer" : nullptr;
  return launch_dyn_scale<mdt::k_dyn_scale_rows>("mdt_dyn_scale_rows", refuse, x, pred, scale, c_skip, c_out, q, B, C, L, Cp, stream);
}

int mdt_loss_rows(const float* x0, const float* x_noisy, const float* pred, const float* c_skip, const float* c_out,
                  const float* weight, const float* dyn_scale, float* loss, int32_t B, int32_t C, int32_t L, int32_t Cp,
                  void* stream) {
  const char* refuse = !x0 || !x_noisy || !pred || !c_skip || !c_out || !weight || !loss ? ": null pointer" : nullptr;
  if (!refuse && (int64_t)C * L > 32768) refuse = ": C * L exceeds 32768 values";
  return launch_tile<mdt::k_loss_rows>("mdt_loss_rows", refuse, B, C, L, Cp, stream, x0, x_noisy, pred, c_skip, c_out, weight,
                                       dyn_scale, loss, C, L, Cp);
}

int mdt_adpm2_mid(const float* x, const float* pred, float* x_mid, float* xin_mid, float c_skip, float c_out,
                  float sigma, float dt_mid, float c_in_mid, int32_t B, int32_t C, int32_t L, int32_t Cp,
                  const float* dyn_scale, void* stream) {
  return launch_tile<mdt::k_adpm2_mid>("mdt_adpm2_mid", nullptr, B, C, L, Cp, stream, x, pred, x_mid, xin_mid, c_skip, c_out, sigma,
                                       dt_mid, c_in_mid, C, L, Cp, dyn_scale);
}

int mdt_adpm2_next(float* x, const float* x_mid, const float* pred, const float* noise, float* xin_next, float c_skip,
                   float c_out, float sigma_mid, float dt_down, float sigma_up, float c_in_next, uint64_t seed,
                   uint32_t step, int64_t sample0, int32_t B, int32_t C, int32_t L, int32_t Cp, int32_t* tokens,
                   const float* dyn_scale, void* stream) {
  const char* refuse = tokens && xin_next ? ": tokens are decoded on the LAST update of a call (xin_next == NULL)" : nullptr;
  return launch_tile<mdt::k_adpm2_next>("mdt_adpm2_next", refuse, B, C, L, Cp, stream, x, x_mid, pred, noise, xin_next, c_skip,
                                        c_out, sigma_mid, dt_down, sigma_up, c_in_next, seed, step, sample0, C, L, Cp, tokens,
                                        dyn_scale);
}

int mdt_aeuler_next(float* x, const float* pred, const float* noise, float* xin_next, float c_skip, float c_out, float sigma,
                    float dt, float sigma_up, float c_in_next, uint64_t seed, uint32_t step, int64_t sample0, int32_t B,
                    int32_t C, int32_t L, int32_t Cp, int32_t* tokens, const float* dyn_scale, void* stream) {
  const char* refuse = !x || !pred ? ": null pointer" : nullptr;
  if (!refuse && tokens && xin_next) refuse = ": tokens are decoded on the LAST update of a call (xin_next == NULL)";
  return launch_tile<mdt::k_aeuler_next>("mdt_aeuler_next", refuse, B, C, L, Cp, stream, x, pred, noise, xin_next, c_skip, c_out,
                                         sigma, dt, sigma_up, c_in_next, seed, step, sample0, C, L, Cp, tokens, dyn_scale);
}

int mdt_karras_hat(const float* x, const float* noise, float* x_hat, float* xin, float noise_scale, float s_noise,
                   float c_in_hat, uint64_t seed, uint32_t step, int64_t sample0, int32_t B, int32_t C, int32_t L,
                   int32_t Cp, void* stream) {
  const char* refuse = !x || !x_hat || !xin ? ": null pointer" : nullptr;
  return launch_tile<mdt::k_karras_hat>("mdt_karras_hat", refuse, B, C, L, Cp, stream, x, noise, x_hat, xin, noise_scale, s_noise,
                                        c_in_hat, seed, step, sample0, C, L, Cp);
}

int mdt_karras_mid(const float* x_hat, const float* pred, float* d, float* x_next, float* xin_next, float c_skip,
                   float c_out, float sigma_hat, float dt, float c_in_next, int32_t B, int32_t C, int32_t L, int32_t Cp,
                   int32_t* tokens, const float* dyn_scale, void* stream) {
  const char* refuse = !x_hat || !pred || !d || !x_next ? ": null pointer" : nullptr;
  if (!refuse && (x_next == x_hat || d == x_hat || d == x_next)) refuse = ": x_hat, d and x_next are three buffers";
  if (!refuse && tokens && xin_next) refuse = ": tokens are decoded when the Euler move ends the call (xin_next == NULL)";
  return launch_tile<mdt::k_karras_mid>("mdt_karras_mid", refuse, B, C, L, Cp, stream, x_hat, pred, d, x_next, xin_next, c_skip,
                                        c_out, sigma_hat, dt, c_in_next, C, L, Cp, tokens, dyn_scale);
}

int mdt_karras_next(const float* x_hat, const float* x_next, const float* d, const float* pred, float* x, float c_skip,
                    float c_out, float sigma_next, float half, int32_t B, int32_t C, int32_t L, int32_t Cp,
                    int32_t* tokens, const float* dyn_scale, void* stream) {
  const char* refuse = !x_hat || !x_next || !d || !pred || !x ? ": null pointer" : nullptr;
  if (!refuse && sigma_next == 0.0f) refuse = ": sigma_next == 0 has no correction (the Euler move is the step)";
  return launch_tile<mdt::k_karras_next>("mdt_karras_next", refuse, B, C, L, Cp, stream, x_hat, x_next, d, pred, x, c_skip, c_out,
                                         sigma_next, half, C, L, Cp, tokens, dyn_scale);
}

int mdt_init_noise(float* x, const float* noise, float sigma0, uint64_t seed, uint32_t step, int64_t sample0, int32_t B,
                   int32_t C, int32_t L, void* stream) {
  if (B <= 0) return 0;
  if (L % 4) return mdt_bad("mdt_init_noise: L % 4 != 0");
  const int64_t n4 = (int64_t)B * C * L / 4;
  hipLaunchKernelGGL(mdt::k_init_noise, dim3(mdt::grid_for(n4)), dim3(256), 0, (hipStream_t)stream, x, noise, sigma0,
                     seed, step, sample0 * C * L, n4);
  return mdt_finish("mdt_init_noise");
}

int mdt_add_noise(float* x, const float* noise, float s, uint64_t seed, uint32_t step, int64_t sample0, int32_t B,
                  int32_t C, int32_t L, void* stream) {
  if (B <= 0) return 0;
  if (L % 4) return mdt_bad("mdt_add_noise: L % 4 != 0");
  const int64_t n4 = (int64_t)B * C * L / 4;
  hipLaunchKernelGGL(mdt::k_add_noise, dim3(mdt::grid_for(n4)), dim3(256), 0, (hipStream_t)stream, x, noise, s, seed,
                     step, sample0 * C * L, n4);
  return mdt_finish("mdt_add_noise");
}

int mdt_inpaint_merge(float* x, const float* src, const uint8_t* mask, const float* noise, float sigma, uint64_t seed,
                      uint32_t step, int64_t sample0, int32_t B, int32_t C, int32_t L, void* stream) {
  if (B <= 0) return 0;
  if (L % 4) return mdt_bad("mdt_inpaint_merge: L % 4 != 0");
  const int64_t n4 = (int64_t)B * C * L / 4;
  hipLaunchKernelGGL(mdt::k_inpaint_merge, dim3(mdt::grid_for(n4)), dim3(256), 0, (hipStream_t)stream, x, src, mask,
                     noise, sigma, seed, step, sample0 * C * L, n4);
  return mdt_finish("mdt_inpaint_merge");
}

int mdt_inpaint_enter(float* x, float* xin, const float* src, const int32_t* draft, const uint8_t* keep,
                      int32_t keep_per_token, const float* n_src, const float* n_re, float sigma, float renoise, float c_in,
                      uint64_t seed, uint32_t step_src, uint32_t step_re, int64_t sample0, int32_t B, int32_t C, int32_t L,
                      int32_t Cp, void* stream) {
  const char* refuse = !x || !xin || !keep ? ": null pointer" : nullptr;
  if (!refuse && !src == !draft) refuse = ": give the source either dense (src) or as draft ids (draft)";
  return launch_tile<mdt::k_inpaint_enter>("mdt_inpaint_enter", refuse, B, C, L, Cp, stream, x, xin, src, draft, keep,
                                           keep_per_token ? 1 : 0, n_src, n_re, sigma, renoise, c_in, seed, step_src, step_re,
                                           sample0, C, L, Cp);
}

int mdt_refine_enter(float* x, float* xin, const int32_t* start, int32_t step_i, const float* src, const int32_t* draft,
                     const float* noise, float sigma, float c_in, uint64_t seed, uint32_t step, int64_t sample0, int32_t B,
                     int32_t C, int32_t L, int32_t Cp, void* stream) {
  const char* refuse = !x || !xin || !start ? ": null pointer" : nullptr;
  if (!refuse && !src == !draft) refuse = ": give the source either dense (src) or as draft ids (draft)";
  return launch_tile<mdt::k_refine_enter>("mdt_refine_enter", refuse, B, C, L, Cp, stream, x, xin, start, step_i, src, draft, noise,
                                          sigma, c_in, seed, step, sample0, C, L, Cp);
}

int mdt_refine_keep_enter(float* x, float* xin, const int32_t* start, int32_t step_i, const float* src, const int32_t* draft,
                          const uint8_t* keep, int32_t keep_per_token, const float* n_entry, const float* n_src, float sigma,
                          float c_in, uint64_t seed, uint32_t step_entry, uint32_t step_src, int64_t sample0, int32_t B, int32_t C,
                          int32_t L, int32_t Cp, void* stream) {
  const char* refuse = !x || !xin || !start || !keep ? ": null pointer" : nullptr;
  if (!refuse && !src == !draft) refuse = ": give the source either dense (src) or as draft ids (draft)";
  return launch_tile<mdt::k_refine_keep_enter>("mdt_refine_keep_enter", refuse, B, C, L, Cp, stream, x, xin, start, step_i, src,
                                               draft, keep, keep_per_token ? 1 : 0, n_entry, n_src, sigma, c_in, seed, step_entry,
                                               step_src, sample0, C, L, Cp);
}

int mdt_inpaint_finish(float* x, const float* src, const int32_t* draft, const uint8_t* keep, int32_t keep_per_token,
                       int32_t* tokens, int32_t B, int32_t C, int32_t L, void* stream) {
  if (B <= 0) return 0;
  if (!x || !keep) return mdt_bad("mdt_inpaint_finish: null pointer");
  if (!src == !draft) return mdt_bad("mdt_inpaint_finish: give the source either dense (src) or as draft ids (draft)");
  if (C <= 0 || L <= 0) return mdt_bad("mdt_inpaint_finish: bad dims");
  const int64_t n = (int64_t)B * L;
  hipLaunchKernelGGL(mdt::k_inpaint_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, src, draft,
                     keep, keep_per_token ? 1 : 0, tokens, B, C, L);
  return mdt_finish("mdt_inpaint_finish");
}

int mdt_adpm2_euler(const float* x_base, const float* x_from, const float* denoised, const float* noise, float* out,
                    float sigma, float dt, float sigma_up, int32_t noise_mode, uint64_t seed, uint32_t step,
                    int64_t sample0, int32_t B, int32_t C, int32_t L, void* stream) {
  if (B <= 0) return 0;
  if (L % 4) return mdt_bad("mdt_adpm2_euler: L % 4 != 0");
  if (noise_mode < 0 || noise_mode > 2 || (noise_mode == 1 && !noise)) return mdt_bad("mdt_adpm2_euler: bad noise mode");
  const int64_t n4 = (int64_t)B * C * L / 4;
  hipLaunchKernelGGL(mdt::k_adpm2_euler, dim3(mdt::grid_for(n4)), dim3(256), 0, (hipStream_t)stream, x_base, x_from,
                     denoised, noise, out, sigma, dt, sigma_up, noise_mode, seed, step, sample0 * C * L, n4);
  return mdt_finish("mdt_adpm2_euler");
}

int mdt_copy_f32(float* dst, const float* src, int64_t n, void* stream) {
  if (n <= 0) return 0;
  if (!dst || !src) return mdt_bad("mdt_copy_f32: null pointer");
  const bool vec = n % 4 == 0 && ((reinterpret_cast<size_t>(dst) | reinterpret_cast<size_t>(src)) & 15) == 0;
  const int64_t items = vec ? n / 4 : (n < 65536 ? n : 65536);
  hipLaunchKernelGGL(mdt::k_copy_f32, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dst, src, n, vec ? 1 : 0);
  return mdt_finish("mdt_copy_f32");
}

int mdt_clamp(float* x, float lo, float hi, int64_t n, void* stream) {
  if (n <= 0) return 0;
  if (n % 4) return mdt_bad("mdt_clamp: n % 4 != 0");
  hipLaunchKernelGGL(mdt::k_clamp, dim3(mdt::grid_for(n / 4)), dim3(256), 0, (hipStream_t)stream, x, lo, hi, n / 4);
  return mdt_finish("mdt_clamp");
}

int mdt_cfg_mix(const float* cond, const float* uncond, float* out, float scale, int64_t n, void* stream) {
  if (n <= 0) return 0;
  if (n % 4) return mdt_bad("mdt_cfg_mix: n % 4 != 0");
  hipLaunchKernelGGL(mdt::k_cfg_mix, dim3(mdt::grid_for(n / 4)), dim3(256), 0, (hipStream_t)stream, cond, uncond, out,
                     scale, n / 4);
  return mdt_finish("mdt_cfg_mix");
}

int mdt_cfg_mix_rows(const float* cond, const float* uncond, float* out, const float* scale, int32_t B, int64_t row_elems,
                     void* stream) {
  if (B <= 0) return 0;
  if (!cond || !uncond || !out || !scale) return mdt_bad("mdt_cfg_mix_rows: null pointer");
  if (row_elems <= 0 || row_elems % 4) return mdt_bad("mdt_cfg_mix_rows: row_elems must be a positive multiple of 4");
  const int64_t row4 = row_elems / 4;
  int G = 256;                                          // lanes of a segment: the power of two that covers a short row
  while (G > 1 && G / 2 >= row4) G /= 2;
  const int64_t segs = (row4 + G - 1) / G, units = (int64_t)B * segs;
  hipLaunchKernelGGL(mdt::k_cfg_mix_rows, dim3(mdt::grid_for(units * G)), dim3(256), 0, (hipStream_t)stream, cond, uncond, out,
                     scale, row4, segs, units, G);
  return mdt_finish("mdt_cfg_mix_rows");
}

int mdt_argmax_tokens(const float* x, int32_t* tokens, int32_t B, int32_t C, int32_t L, void* stream) {
  if (B <= 0) return 0;
  const int64_t n = (int64_t)B * L;
  hipLaunchKernelGGL(mdt::k_argmax, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, tokens, B,
                     C, L);
  return mdt_finish("mdt_argmax_tokens");
}

}  // extern "C"
