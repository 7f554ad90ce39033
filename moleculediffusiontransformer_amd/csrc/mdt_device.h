// Device primitives shared by the ring and block kernels (k_tblock_lw, k_tblock32, k_tf128, k_tf256, k_rconv, k_res256, k_proj,
// k_resblock, k_attn): vector types, MFMA names, lane-group exchanges, operand splits, counted LDS reads and their waits; and by the
// screening and molecule kernels (k_screen, k_edit, k_mol*): the 64-bit shuffle and lane reads, the edit-distance recurrence, the
// wave-local LDS ordering.  (What the molecule kernels share about the graph row itself is mdt_molrow.h's.)
// Device code only; included by the .hip files that use it, never through mdt_kernels.h (mdt_api.cpp does not see it).
// Everything is __forceinline__: a kernel's code object does not depend on whether a primitive is defined here or in its file.
// The rule: a primitive used by two kernels lives here, once, with its rationale; what one kernel alone uses stays in its file.
#pragma once

#include <hip/hip_runtime.h>

#define MDT_MFMA_BF16 __builtin_amdgcn_mfma_f32_16x16x32_bf16
#define MDT_MFMA_F32 __builtin_amdgcn_mfma_f32_16x16x4f32
#define MDT_MFMA_F32_BLK __builtin_amdgcn_mfma_f32_4x4x1f32   // 16 independent 4 x 4 x 1 blocks (block = lane >> 2), same exact fp32 products

// ring slot of tile t (run-time t; NS = the including file's slot count, a power of two): a mask, not the signed modulo
// (7 scalar instructions per use)
#ifdef MDT_SLOT_MOD
#define MDT_SLOT_IDX(t) ((t) % NS)
#else
#define MDT_SLOT_IDX(t) ((t) & (NS - 1))
#endif

namespace mdt {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(4))) const unsigned* cu32p;   // constant address space: scalar loads

// streaming store: the output is consumed by the next launch (through the memory side: the per-XCD L2s are written
// back / invalidated at every kernel boundary anyway), so it need not stay dirty in this XCD's L2 until kernel end
__device__ __forceinline__ void store_nt(float* p, float4 v) {
  typedef float f4 __attribute__((ext_vector_type(4)));
  __builtin_nontemporal_store(f4{v.x, v.y, v.z, v.w}, reinterpret_cast<f4*>(p));
}

// lane-group exchanges over +-16 / +-32 lanes with the gfx950 permlane swaps (VALU, no LDS round trip). The swap is in
// place on two registers: fed the same value twice, v_permlane16_swap leaves (rows 0,0,2,2) and (rows 1,1,3,3),
// v_permlane32_swap (halves lo,lo) and (hi,hi); combining the two gives every lane the pair it would get from xor 16 /
// xor 32. Written as asm: through __builtin_amdgcn_permlane*_swap hipcc 7.2 folds the two results into one register.
// The s_nop covers the VALU-write -> permlane-swap-read hazard for the copies the compiler places just before.
#define MDT_XG(NAME, INSN, COMBINE)                                                      \
  __device__ __forceinline__ float NAME(float v) {                                       \
    float a = v, b = v;                                                                  \
    asm("s_nop 1\n\t" INSN " %0, %1" : "+v"(a), "+v"(b));                                \
    return COMBINE;                                                                      \
  }
MDT_XG(xg16_add, "v_permlane16_swap_b32", a + b)
MDT_XG(xg32_add, "v_permlane32_swap_b32", a + b)
MDT_XG(xg16_max, "v_permlane16_swap_b32", fmaxf(a, b))
MDT_XG(xg32_max, "v_permlane32_swap_b32", fmaxf(a, b))
#undef MDT_XG

// The same swaps fed TWO values: a reduce-scatter step (each half of the lane pair keeps the sum of one value) and an all-gather
// step (both lanes of the pair get both values, in the pair's order).  v_permlane32_swap_b32 a, b exchanges lanes 32-63 of a with
// lanes 0-31 of b; v_permlane16_swap_b32 the odd 16-lane rows of a with the even rows of b.
__device__ __forceinline__ float rs32_add(float x, float y) {   // lanes 0-31: x + (x of lane + 32); lanes 32-63: (y of lane - 32) + y
  asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(x), "+v"(y));
  return x + y;
}
__device__ __forceinline__ float rs16_add(float x, float y) {   // even rows: x + (x of lane + 16); odd rows: (y of lane - 16) + y
  asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(x), "+v"(y));
  return x + y;
}
__device__ __forceinline__ void ag32(float v, float& lo, float& hi) {       // lo / hi: v of the pair's lane in lanes 0-31 / 32-63
  lo = v; hi = v;
  asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(lo), "+v"(hi));
}
__device__ __forceinline__ void ag16(float v, float& even, float& odd) {    // even / odd: v of the pair's lane in the even / odd row
  even = v; odd = v;
  asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(even), "+v"(odd));
}

__device__ __forceinline__ float gelu(float x) {   // exact-erf GELU, branch-free erf (A&S 7.1.26, |error| < 1.5e-7)
  const float z = fabsf(x) * 0.70710678118654752440f;
  const float t = __builtin_amdgcn_rcpf(1.0f + 0.3275911f * z);
  const float poly = t * (0.254829592f + t * (-0.284496736f + t * (1.421413741f + t * (-1.453152027f + t * 1.061405429f))));
  const float erfa = 1.0f - poly * __expf(-z * z);
  return 0.5f * x * (1.0f + copysignf(erfa, x));
}

// SiLU as the tiled GEMMs' prologues apply it: full-precision division and expf (the fused block kernels keep their own
// v_rcp / __expf form)
__device__ __forceinline__ float silu_exact(float x) { return x / (1.0f + expf(-x)); }

// Two values -> their packed bf16 hi halves and packed bf16 lo halves (v = hi + lo to 2^-17), both rounded to nearest: one
// v_cvt_pk_bf16_f32 for the pair's hi, a shift and a mask to widen them back, two subtractions, one v_cvt_pk_bf16_f32 for the lo --
// 6 VALU instructions per pair (5 where the compiler packs the subtractions).  Written pairwise on purpose: from the per-element
// form `h = (__bf16)v; lo = (__bf16)(v - (float)h)` hipcc 7.2 converts about a third of the values twice (once alone for the
// subtraction, once packed for the operand), 8 instructions per pair.  Same roundings, same bits.
__device__ __forceinline__ void split2(float a, float b, unsigned& hi, unsigned& lo) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  hi = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{a, b}, bf16x2));
  const float la = a - __uint_as_float(hi << 16), lb = b - __uint_as_float(hi & 0xffff0000u);
  lo = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{la, lb}, bf16x2));
}

// 8 values of one k-step -> the two 128-bit operand registers of the step.  Split-bf16 products (F32 = false): bf16 hi plane /
// lo plane (v = hi + lo to 2^-17).  Exact fp32 products (F32 = true): the values themselves, slots e = 0..3 in `hi`, 4..7 in
// `lo` (bit casts: the operand arrays keep one type for both instantiations; an fp32 k-step is eight 16x16x4 MFMAs, slot
// (g, e = 4 lo + r) of the bf16 step being contraction index g of MFMA (lo, r))
template <bool F32>
__device__ __forceinline__ void split8(const float v[8], bf16x8& hi, bf16x8& lo) {
  if constexpr (F32) {
    hi = __builtin_bit_cast(bf16x8, f32x4{v[0], v[1], v[2], v[3]});
    lo = __builtin_bit_cast(bf16x8, f32x4{v[4], v[5], v[6], v[7]});
  } else {
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    u32x4 h, l;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      unsigned hh, ll;
      split2(v[2 * p], v[2 * p + 1], hh, ll);
      h[p] = hh;
      l[p] = ll;
    }
    hi = __builtin_bit_cast(bf16x8, h);
    lo = __builtin_bit_cast(bf16x8, l);
  }
}

// 4 values -> their bf16 hi / lo planes (8-byte LDS writes of an activation row; the 4 k-slots of a 16-key MFMA operand)
__device__ __forceinline__ void split4(const float v[4], bf16x4& hi, bf16x4& lo) {
  typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
  u32x2 h, l;
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    unsigned hh, ll;
    split2(v[2 * p], v[2 * p + 1], hh, ll);
    h[p] = hh;
    l[p] = ll;
  }
  hi = __builtin_bit_cast(bf16x4, h);
  lo = __builtin_bit_cast(bf16x4, l);
}

__device__ __forceinline__ unsigned lds_addr(const unsigned char* p) {
  return (unsigned)(size_t)(__attribute__((address_space(3))) const unsigned char*)p;
}

// 16-byte LDS read, whole address in the register.  The reads are asm volatile: they stay where they are written, between
// the MFMAs that hide them, and the kernels count them themselves (lgkm_wait)
__device__ __forceinline__ void lds_read16(bf16x8& dst, const unsigned char* p) {
  const unsigned addr = (unsigned)(size_t)(__attribute__((address_space(3))) const unsigned char*)p;
  asm volatile("ds_read_b128 %0, %1" : "=v"(dst) : "v"(addr) : "memory");
}

// fragment read with the (tile, plane) part of the address in the instruction's immediate offset: per read there is no
// address arithmetic left (one v_add_u32 per ds_read_b128 was 127 of the 679 instructions of a self-attention head,
// in a kernel whose compute waves are issue-bound)
template <int OFF>
__device__ __forceinline__ void lds_read16_off(bf16x8& dst, unsigned addr) {
  static_assert(OFF >= 0 && OFF < 65536, "ds_read_b128 offset field");
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF) : "memory");
}

// per-head bias vectors live in LDS behind the ring and are read like fragments (asm, counted in the lgkmcnt waits): a
// global load issued by a compute wave queues behind the loader waves' DMA traffic and stalls its issue ~60 cycles
template <int OFF>
__device__ __forceinline__ void lds_read_f4_off(f32x4& dst, unsigned addr) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF) : "memory");
}

// at most N LDS/scalar operations still in flight; the sched_barrier keeps the compiler from moving the MFMAs that
// consume the awaited fragments across the wait.  Two tiers, the two that the kernels use.
template <int N>
__device__ __forceinline__ void lgkm_wait() {
  static_assert(N == 0 || N == 4, "lgkm_wait has the tiers lgkmcnt(0) and lgkmcnt(4) only");
  if constexpr (N >= 4) asm volatile("s_waitcnt lgkmcnt(4)" ::: "memory");
  else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}

// operand of the neighbouring token row: lane i takes lane i - 1 (SHR) or i + 1 inside its 16-lane row, 0 at the ends
// (DPP row_shr / row_shl with zero fill); keep = false also zeroes it (sample boundaries inside the row)
template <bool SHR>
__device__ __forceinline__ bf16x8 row_shift(const bf16x8& v, bool keep) {
  const i32x4 s = __builtin_bit_cast(i32x4, v);
  i32x4 r;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int t = __builtin_amdgcn_update_dpp(0, s[k], SHR ? 0x111 : 0x101, 0xf, 0xf, true);
    r[k] = keep ? t : 0;
  }
  return __builtin_bit_cast(bf16x8, r);
}

// What one lane wrote to LDS is read by other lanes of the SAME wave (k_molfp: the labels and the fingerprint of a row; k_molsub:
// the adjacency columns, the compat words and the found word of a row): order the accesses.  The waves of these workgroups each
// own a row and its slice of LDS, so a workgroup barrier would couple waves that share nothing -- and could not be reached from
// their wave-uniform, per-row control flow.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// 64-bit butterfly exchange over the wave as two 32-bit shuffles (k_screen: the row key; k_molgraph: the sum over the roots)
__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int off) {
  const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, off, 64);
  const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), off, 64);
  return ((unsigned long long)hi << 32) | lo;
}

// One lane's value as a wave-uniform (scalar) value (k_molwrite: the walks over rank and seq; k_molcanon: the twins, the entries, the
// components).  lane: the same in every lane, though the compiler may not know it -- hence the readfirstlane.
__device__ __forceinline__ uint64_t readlane_u64(uint64_t v, int lane) {
  const int at = __builtin_amdgcn_readfirstlane(lane);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, at);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), at);
  return (uint64_t)hi << 32 | lo;
}
__device__ __forceinline__ int readlane_i32(int v, int lane) {
  return __builtin_amdgcn_readlane(v, __builtin_amdgcn_readfirstlane(lane));
}
// v is the same in every lane: tell the compiler so (a word read from LDS that steers wave-uniform control flow)
__device__ __forceinline__ uint64_t uniform_u64(uint64_t v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
  return (uint64_t)hi << 32 | lo;
}

// Levenshtein distance by Hyyro's form of Myers' bit-vector recurrence (k_edit, k_screen): the pattern a[0:m], 1 <= m <= 64, is
// the match masks Peq[s] (bit j set when a[j] == s); column after column of the dynamic programme is then one text symbol each.
// State: pv = ~0, mv = 0, distance = m; per text symbol  distance += edit_step(Peq[symbol], edit_top(m), pv, mv).
// An id outside [0, 64) has no mask: the caller passes eq = 0 for it (edit_has_mask), so it matches nothing, itself included.
// Bits above m - 1 never reach the bits below them (carries and shifts go upwards), so no mask of the low m bits is needed and
// m == 64 shifts by nothing: the only place the length enters is the probe bit.  m == 0 has no probe bit: edit_top gives 0, the
// steps count nothing, and the caller takes the text's length as the distance.
__device__ __forceinline__ unsigned long long edit_top(int m) { return m > 0 ? 1ull << (m - 1) : 0ull; }

__device__ __forceinline__ bool edit_has_mask(int id) { return (unsigned)id < 64u; }

__device__ __forceinline__ int edit_step(unsigned long long eq, unsigned long long top, unsigned long long& pv,
                                         unsigned long long& mv) {
  const unsigned long long xv = eq | mv;
  const unsigned long long xh = (((eq & pv) + pv) ^ pv) | eq;
  unsigned long long ph = mv | ~(xh | pv);
  unsigned long long mh = pv & xh;
  const int delta = (int)((ph & top) != 0) - (int)((mh & top) != 0);
  ph = (ph << 1) | 1ull;                                          // (the top boundary row of a GLOBAL distance grows by one a column)
  mh <<= 1;
  pv = mh | ~(xv | ph);
  mv = ph & xv;
  return delta;
}

}  // namespace mdt
