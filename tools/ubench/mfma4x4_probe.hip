// v_mfma_f32_4x4x1_16b_f32 (__builtin_amdgcn_mfma_f32_4x4x1f32) on gfx950: the operand map, checked on random fp32 data against the
// host, and the cycles per instruction back to back (independent accumulators) and on one dependent accumulator chain.
//   map under test:  A (1 VGPR): lane l holds A[block l / 4][row l % 4]
//                    B (1 VGPR): lane l holds B[block l / 4][col l % 4]
//                    D (4 VGPRs): register r of lane l holds D[block l / 4][row r][col l % 4] = C + A[row r] * B[col l % 4]
//   hipcc -O3 --offload-arch=gfx950 tools/ubench/mfma4x4_probe.hip -o tools/ubench/bin/mfma4x4_probe && tools/ubench/bin/mfma4x4_probe
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
typedef float f32x4 __attribute__((ext_vector_type(4)));

__global__ void k_map(const float* a, const float* b, const float* c, float* d, int steps) {
  const int l = threadIdx.x;
  f32x4 acc = f32x4{c[4 * l], c[4 * l + 1], c[4 * l + 2], c[4 * l + 3]};
  for (int s = 0; s < steps; ++s) acc = __builtin_amdgcn_mfma_f32_4x4x1f32(a[64 * s + l], b[64 * s + l], acc, 0, 0, 0);
  for (int r = 0; r < 4; ++r) d[4 * l + r] = acc[r];
}

template <int NACC>
__global__ void k_rate(const float* in, float* out, unsigned long long* cyc, int iters) {
  float a[8], b[8];
  for (int e = 0; e < 8; ++e) { a[e] = in[threadIdx.x + e]; b[e] = in[threadIdx.x + 64 + e]; }
  f32x4 acc[NACC];
  for (int n = 0; n < NACC; ++n) acc[n] = f32x4{0, 0, 0, 0};
  unsigned long long t0, t1;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t0)::"memory");
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int r = 0; r < 64 / NACC; ++r)
#pragma unroll
      for (int n = 0; n < NACC; ++n)
        acc[n] = __builtin_amdgcn_mfma_f32_4x4x1f32(a[(r * NACC + n) % 8], b[(r * NACC + n) % 8], acc[n], 0, 0, 0);
  }
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t1)::"memory");
  f32x4 s = acc[0];
  for (int n = 1; n < NACC; ++n) s += acc[n];
  out[blockIdx.x * blockDim.x + threadIdx.x] = s[0] + s[1] + s[2] + s[3];
  if (threadIdx.x == 0 && blockIdx.x == 0) cyc[0] = t1 - t0;
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

template <int NACC>
int rate(const float* in, float* out, unsigned long long* cyc, int threads, const char* what) {
  const int iters = 200;
  for (int rep = 0; rep < 2; ++rep) hipLaunchKernelGGL((k_rate<NACC>), dim3(256), dim3(threads), 0, 0, in, out, cyc, iters);
  CK(hipDeviceSynchronize());
  unsigned long long c;
  CK(hipMemcpy(&c, cyc, 8, hipMemcpyDeviceToHost));
  printf("%-24s %2d accumulator(s): %7llu shader cycles for %d MFMAs = %.1f cycles per MFMA\n", what, NACC, c, 64 * iters, (double)c / (64.0 * iters));
  return 0;
}

int main() {
  const int steps = 5;
  float ha[64 * steps], hb[64 * steps], hc[256], hd[256];
  srand(7);
  for (int e = 0; e < 64 * steps; ++e) { ha[e] = rand() / (float)RAND_MAX - 0.5f; hb[e] = rand() / (float)RAND_MAX - 0.5f; }
  for (int e = 0; e < 256; ++e) hc[e] = rand() / (float)RAND_MAX - 0.5f;
  float *a, *b, *c, *d, *in, *out; unsigned long long* cyc;
  CK(hipMalloc(&a, sizeof ha)); CK(hipMalloc(&b, sizeof hb)); CK(hipMalloc(&c, sizeof hc)); CK(hipMalloc(&d, sizeof hd));
  CK(hipMalloc(&in, 4096 * 4)); CK(hipMalloc(&out, 256 * 512 * 4)); CK(hipMalloc(&cyc, 8));
  CK(hipMemcpy(a, ha, sizeof ha, hipMemcpyHostToDevice)); CK(hipMemcpy(b, hb, sizeof hb, hipMemcpyHostToDevice));
  CK(hipMemcpy(c, hc, sizeof hc, hipMemcpyHostToDevice)); CK(hipMemset(in, 0, 4096 * 4));
  hipLaunchKernelGGL(k_map, dim3(1), dim3(64), 0, 0, a, b, c, d, steps);
  CK(hipDeviceSynchronize());
  CK(hipMemcpy(hd, d, sizeof hd, hipMemcpyDeviceToHost));
  // the map under test, and its transpose (register = column, lane = row) for the report
  int bad = 0, bad_t = 0, bitwise = 0;
  for (int l = 0; l < 64; ++l)
    for (int r = 0; r < 4; ++r) {
      const int blk = l >> 2, j = l & 3;
      float e = hc[4 * l + r], et = hc[4 * l + r];
      for (int s = 0; s < steps; ++s) {
        e = fmaf(ha[64 * s + 4 * blk + r], hb[64 * s + 4 * blk + j], e);
        et = fmaf(ha[64 * s + 4 * blk + j], hb[64 * s + 4 * blk + r], et);
      }
      bad += fabsf(hd[4 * l + r] - e) > 1e-6f;
      bad_t += fabsf(hd[4 * l + r] - et) > 1e-6f;
      bitwise += hd[4 * l + r] == e;
    }
  printf("operand map: %d of 256 results off under the map in the header (%d bitwise equal to an fmaf chain in step order), %d off under its transpose\n",
         bad, bitwise, bad_t);
  if (rate<1>(in, out, cyc, 256, "1 wave/SIMD, dependent")) return 1;
  if (rate<2>(in, out, cyc, 256, "1 wave/SIMD")) return 1;
  if (rate<4>(in, out, cyc, 256, "1 wave/SIMD")) return 1;
  if (rate<8>(in, out, cyc, 256, "1 wave/SIMD")) return 1;
  if (rate<4>(in, out, cyc, 512, "2 waves/SIMD")) return 1;
  return bad != 0;
}
