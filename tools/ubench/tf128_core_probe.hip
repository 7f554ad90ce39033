// The attention core of one k_tf128 head (a wave's 16 rows against 16 keys, 64 features; csrc/k_tf128.hip), exact fp32 form against
// the split-bf16 form, one wave per SIMD on every CU, random operands in registers:
//   form 0:  S^T and O^T on v_mfma_f32_16x16x4_f32 (16 + 16 MFMAs)                                   -- the exact mode's core
//   form 1:  q, k, v, p split to bf16 hi / lo; S^T 6 x v_mfma_f32_16x16x32_bf16, O^T 12 x v_mfma_f32_16x16x16_bf16  -- the default mode's
//   form 2:  as 1 with O^T on 12 x v_mfma_f32_16x16x32_bf16, upper 4 k-slots zero
// Each iteration is one head: scores, scale, maximum, exp2, sum, rcp, P V, and the hi / lo split of the 16 outputs that the O
// phase behind the core consumes; the outputs feed the next iteration's q so that nothing is hoisted.  Reported: shader cycles per
// head (s_memtime of workgroup 0), the clock held (s_memtime / s_memrealtime x 100 MHz) and the wall time per head (events).
//   hipcc -O3 --offload-arch=gfx950 -mllvm -amdgpu-mfma-vgpr-form=1 -Imoleculediffusiontransformer_amd/csrc \
//     tools/ubench/tf128_core_probe.hip -o tools/ubench/bin/tf128_core_probe && tools/ubench/bin/tf128_core_probe
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "mdt_device.h"
using namespace mdt;

typedef short s16x4 __attribute__((ext_vector_type(4)));

template <int FORM>
__device__ __forceinline__ void head(const f32x4* qT, const f32x4* kT, const f32x4* vT, float scale2, f32x4* oT) {
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 s = zero4;
  bf16x4 vh[4], vl[4];
  if constexpr (FORM == 0) {
    f32x4 s1 = zero4;
#pragma unroll
    for (int ft = 0; ft < 4; ++ft) {
      s = MDT_MFMA_F32(kT[ft][0], qT[ft][0], s, 0, 0, 0);
      s1 = MDT_MFMA_F32(kT[ft][1], qT[ft][1], s1, 0, 0, 0);
      s = MDT_MFMA_F32(kT[ft][2], qT[ft][2], s, 0, 0, 0);
      s1 = MDT_MFMA_F32(kT[ft][3], qT[ft][3], s1, 0, 0, 0);
    }
    s += s1;
  } else {
#pragma unroll
    for (int sp = 0; sp < 2; ++sp) {
      float kv[8], qv[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        kv[e] = kT[2 * sp + (e >> 2)][e & 3];
        qv[e] = qT[2 * sp + (e >> 2)][e & 3];
      }
      bf16x8 kh, kl, qh, ql;
      split8<false>(kv, kh, kl);
      split8<false>(qv, qh, ql);
      s = MDT_MFMA_BF16(kl, qh, s, 0, 0, 0);
      s = MDT_MFMA_BF16(kh, ql, s, 0, 0, 0);
      s = MDT_MFMA_BF16(kh, qh, s, 0, 0, 0);
    }
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      const float v[4] = {vT[dt][0], vT[dt][1], vT[dt][2], vT[dt][3]};
      split4(v, vh[dt], vl[dt]);
    }
  }
  float st[4], mx = -INFINITY;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    st[r] = s[r] * scale2;
    mx = fmaxf(mx, st[r]);
  }
  mx = xg32_max(xg16_max(mx));
  float sum = 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    st[r] = __builtin_amdgcn_exp2f(st[r] - mx);
    sum += st[r];
  }
  sum = xg32_add(xg16_add(sum));
  const float inv = __builtin_amdgcn_rcpf(sum);
  if constexpr (FORM == 0) {
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) oT[dt] = zero4;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) oT[dt] = MDT_MFMA_F32(vT[dt][r], st[r] * inv, oT[dt], 0, 0, 0);
  } else {
    const float p[4] = {st[0] * inv, st[1] * inv, st[2] * inv, st[3] * inv};
    bf16x4 ph, pl;
    split4(p, ph, pl);
    auto mm = [&](const bf16x4& a, const bf16x4& b, const f32x4& c) __attribute__((always_inline)) {
      if constexpr (FORM == 1) {
        return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(s16x4, a), __builtin_bit_cast(s16x4, b), c, 0, 0, 0);
      } else {
        const bf16x8 a8 = {a[0], a[1], a[2], a[3], 0, 0, 0, 0}, b8 = {b[0], b[1], b[2], b[3], 0, 0, 0, 0};
        return MDT_MFMA_BF16(a8, b8, c, 0, 0, 0);
      }
    };
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) oT[dt] = mm(vl[dt], ph, zero4);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) oT[dt] = mm(vh[dt], pl, oT[dt]);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) oT[dt] = mm(vh[dt], ph, oT[dt]);
  }
}

template <int FORM>
__global__ __launch_bounds__(256) void k_core(const float* in, float* out, unsigned long long* stamps, int iters) {
  const int lane = threadIdx.x & 63;
  f32x4 qT[4], kT[4], vT[4], oT[4];
  const float* p = in + ((blockIdx.x * 4 + (threadIdx.x >> 6)) % 64) * 64 * 48 + lane * 48;   // the host's buffer holds 64 waves' operands
#pragma unroll
  for (int ft = 0; ft < 4; ++ft)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      qT[ft][r] = p[4 * ft + r];
      kT[ft][r] = p[16 + 4 * ft + r];
      vT[ft][r] = p[32 + 4 * ft + r];
    }
  f32x4 accs = {0.f, 0.f, 0.f, 0.f};
  unsigned long long t0, t1, r0, r1;
  asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(t0), "=s"(r0)::"memory");
  for (int it = 0; it < iters; ++it) {
    head<FORM>(qT, kT, vT, 0.125f * 1.44269504f, oT);
    bf16x8 oh[2], ol[2];                             // what the O phase behind the core consumes
#pragma unroll
    for (int sp = 0; sp < 2; ++sp) {
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = oT[2 * sp + (e >> 2)][e & 3];
      split8<false>(v, oh[sp], ol[sp]);
    }
    accs = MDT_MFMA_BF16(oh[0], ol[1], accs, 0, 0, 0);
    accs = MDT_MFMA_BF16(oh[1], ol[0], accs, 0, 0, 0);
#pragma unroll
    for (int ft = 0; ft < 4; ++ft) qT[ft] = qT[ft] * 0.75f + oT[ft] * 0.25f;   // the next head's q depends on this head
  }
  asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(t1), "=s"(r1)::"memory");
  f32x4 s = accs + qT[0] + qT[1] + qT[2] + qT[3];
  out[blockIdx.x * blockDim.x + threadIdx.x] = s[0] + s[1] + s[2] + s[3];
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    stamps[0] = t1 - t0;
    stamps[1] = r1 - r0;
  }
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

template <int FORM>
int run(const float* in, float* out, unsigned long long* stamps, float* first, const char* what) {
  const int iters = 2000, blocks = 256;
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  hipLaunchKernelGGL((k_core<FORM>), dim3(blocks), dim3(256), 0, 0, in, out, stamps, iters);   // warm-up
  CK(hipEventRecord(e0));
  for (int rep = 0; rep < 20; ++rep) hipLaunchKernelGGL((k_core<FORM>), dim3(blocks), dim3(256), 0, 0, in, out, stamps, iters);
  CK(hipEventRecord(e1));
  CK(hipDeviceSynchronize());
  float ms;
  CK(hipEventElapsedTime(&ms, e0, e1));
  unsigned long long st[2];
  CK(hipMemcpy(st, stamps, 16, hipMemcpyDeviceToHost));
  hipLaunchKernelGGL((k_core<FORM>), dim3(1), dim3(256), 0, 0, in, out, stamps + 2, 1);        // one head, for the comparison below
  CK(hipDeviceSynchronize());
  CK(hipMemcpy(first, out, 256 * 4, hipMemcpyDeviceToHost));
  printf("%-44s %7.1f shader cycles per head, clock held %.2f GHz, wall %.3f us per head\n", what, (double)st[0] / iters,
         (double)st[0] / (double)st[1] * 0.1, ms * 1e3 / (20.0 * iters));
  return 0;
}

int main() {
  const int n = 64 * 64 * 48;
  float* h = (float*)malloc(n * 4);
  srand(11);
  for (int e = 0; e < n; ++e) h[e] = 2.f * (rand() / (float)RAND_MAX - 0.5f);
  float *in, *out; unsigned long long* stamps;
  CK(hipMalloc(&in, n * 4)); CK(hipMalloc(&out, 256 * 256 * 4)); CK(hipMalloc(&stamps, 32));
  CK(hipMemcpy(in, h, n * 4, hipMemcpyHostToDevice));
  float o0[256], o1[256], o2[256];
  if (run<0>(in, out, stamps, o0, "fp32 core (32 x 16x16x4 f32)")) return 1;
  if (run<1>(in, out, stamps, o1, "split core (6 x 16x16x32 + 12 x 16x16x16)")) return 1;
  if (run<2>(in, out, stamps, o2, "split core (6 + 12 x 16x16x32, 4 slots zero)")) return 1;
  float d1 = 0.f, d2 = 0.f, m = 0.f;
  for (int e = 0; e < 256; ++e) { d1 = fmaxf(d1, fabsf(o1[e] - o0[e])); d2 = fmaxf(d2, fabsf(o2[e] - o1[e])); m = fmaxf(m, fabsf(o0[e])); }
  printf("per-lane checksum of workgroup 0 after one head: max |split - fp32| = %.3g (|fp32| max %.3g), max |form 2 - form 1| = %.3g\n", d1, m, d2);
  return !(std::isfinite(d1) && std::isfinite(m));
}
