// Candidate screening on gfx950: what the reference's callers do with generated molecules after the forward model has
// re-predicted their properties (sample_loop_generative / generate_from_conditioning, generative.py:1196-1291, :1685-1738) --
// compare with the target, ask is_novel() (:1063), keep the best -- on token ids, without leaving the device.
//
//   k_tokens_compact   ids (B, L) -> non-zero ids left-packed, their number, a 64-bit key of the packed row, and (optionally) the
//                      forward model's input (generative.py:425-429 on ids: tokens_to_forward_input)
//   k_screen_score     weighted mean squared distance of the re-predicted properties from the group's target
//   k_screen_select    per group: status bits (empty / non-finite / duplicate / known) and the K best eligible candidates
//   k_screen_select_diverse   the same with novelty as a distance and the K best that lie min_distance edits apart
// Both selections take an optional per-row `reject` byte (mdt_smiles_check's status) that is OR-ed into the status first; they
// open with the same select_prologue, and their five entry points check and launch through one select_launch.
//
// Rows are r = c * G + g: candidate c of group g (a group is one target conditioning), the layout of guidance_sweep.
// A molecule IS its compacted id row (the reference's string: a character-level tokenizer, id 0 skipped), so equality is decided
// on (length, packed row); the key only spares comparisons and is never trusted on its own.
//
// Built with -ffp-contract=off: the score keeps separate fp32 multiplies and adds, so a numpy fp32 loop reproduces it.
#include "mdt_kernels.h"
#include "mdt_device.h"
#include "../../include/mdt_hip.h"

#include <climits>
#include <cmath>

namespace mdt {

// The key word of packed element j with id `id` (mdt_hip.h, mdt_tokens_compact): one splitmix64 step of (j << 32) | id.
__device__ __forceinline__ uint64_t key_word(uint32_t j, uint32_t id) {
  uint64_t z = (((uint64_t)j << 32) | id) + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// One 64-lane wave per row, four rows per block.  Positions in chunks of 64: ballot the non-zero lanes, the popcount of the lanes
// below is the slot, a running base carries over the chunks.  No LDS.  tokens and packed must not overlap.
__global__ __launch_bounds__(256) void k_tokens_compact(const int32_t* __restrict__ tokens, int B, int L, float* __restrict__ fwd_in,
                                                        int Lf, double x_norm, int32_t* __restrict__ packed,
                                                        int32_t* __restrict__ length, uint64_t* __restrict__ key) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= B) return;                                      // (a whole wave leaves: no barrier, no cross-wave traffic below)
  const int32_t* src = tokens + (int64_t)row * L;
  int32_t* dst = packed + (int64_t)row * L;
  float* fin = fwd_in ? fwd_in + (int64_t)row * Lf : nullptr;
  const uint64_t below = ((uint64_t)1 << lane) - 1;
  int base = 0;
  uint64_t k = 0;
  for (int c0 = 0; c0 < L; c0 += 64) {
    const int p = c0 + lane;
    const int32_t id = p < L ? src[p] : 0;
    const uint64_t mask = __ballot(id != 0);
    if (id != 0) {
      const int slot = base + __popcll(mask & below);
      dst[slot] = id;
      k += key_word((uint32_t)slot, (uint32_t)id);
      if (fin && slot < Lf) fin[slot] = (float)((double)id / x_norm);
    }
    base += __popcll(mask);
  }
  for (int j = base + lane; j < L; j += 64) dst[j] = 0;
  if (fin)
    for (int j = base + lane; j < Lf; j += 64) fin[j] = 0.0f;
  for (int off = 32; off >= 1; off >>= 1) k += shfl_xor_u64(k, off);     // (a sum mod 2^64: exact in any order)
  if (lane == 0) {
    length[row] = base;
    key[row] = k;
  }
}

// One thread per row; i ascending, separate multiply and add.
__global__ __launch_bounds__(256) void k_screen_score(const float* __restrict__ props, int64_t row_stride,
                                                      const float* __restrict__ target, const float* __restrict__ weights, int rows,
                                                      int G, int n, float* __restrict__ score) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const float* p = props + (int64_t)r * row_stride;
  const float* t = target + (int64_t)(r % G) * n;
  float acc = 0.0f;
  for (int i = 0; i < n; ++i) {
    const float d = p[i] - t[i];
    float sq = d * d;
    if (weights) sq = weights[i] * sq;
    acc = acc + sq;
  }
  score[r] = acc / (float)n;
}

constexpr int kScreenMaxN = 1024;

__device__ __forceinline__ bool same_row(const int32_t* a, const int32_t* b, int len) {
  for (int j = 0; j < len; ++j)
    if (a[j] != b[j]) return false;
  return true;
}

// Status bits 1, 2, 4, 8 of candidate c of group g (mdt_hip.h); s_key, s_score, s_len hold the group's N candidates.
__device__ __forceinline__ int candidate_status(int c, int g, int G, int L, const uint64_t* s_key, const float* s_score,
                                                const int32_t* s_len, const int32_t* __restrict__ packed,
                                                const uint64_t* __restrict__ known_key, const int32_t* __restrict__ known_packed,
                                                const int32_t* __restrict__ known_len, int M) {
  const uint64_t k = s_key[c];
  const int len = s_len[c];
  const int32_t* row = packed + ((int64_t)c * G + g) * L;
  int st = 0;
  if (len == 0) st |= MDT_SCREEN_EMPTY;
  if (!isfinite(s_score[c])) st |= MDT_SCREEN_NONFINITE;
  for (int o = 0; o < c; ++o)                                  // the first occurrence stands for the molecule
    if (s_key[o] == k && s_len[o] == len && same_row(row, packed + ((int64_t)o * G + g) * L, len)) {
      st |= MDT_SCREEN_DUPLICATE;
      break;
    }
  if (M > 0) {
    int lo = 0, hi = M;                                        // lower bound of k in known_key (ascending)
    while (lo < hi) {
      const int mid = lo + (hi - lo) / 2;
      if (known_key[mid] < k) lo = mid + 1; else hi = mid;
    }
    for (int i = lo; i < M && known_key[i] == k; ++i)          // the whole run of equal keys
      if (known_len[i] == len && same_row(row, known_packed + (int64_t)i * L, len)) {
        st |= MDT_SCREEN_KNOWN;
        break;
      }
  }
  return st;
}

// The opening of both selections, by the group's whole workgroup: the keys, scores and lengths of its N candidates into LDS; every
// candidate's status -- candidate_status, KNOWN also where known_dist (or nullptr) is below min_novelty, then the `reject` byte (or
// nullptr: a verdict from outside such as mdt_smiles_check's, never eligible) -- into s_status and `status`.  Ends behind a
// barrier; -> the number of eligible candidates (status 0), the same in every thread.
__device__ __forceinline__ int select_prologue(const float* __restrict__ score, const uint64_t* __restrict__ key,
                                               const int32_t* __restrict__ packed, const int32_t* __restrict__ length, int L, int N,
                                               int G, const uint64_t* __restrict__ known_key,
                                               const int32_t* __restrict__ known_packed, const int32_t* __restrict__ known_len, int M,
                                               const int32_t* __restrict__ known_dist, int min_novelty,
                                               const uint8_t* __restrict__ reject, uint8_t* __restrict__ status, uint64_t* s_key,
                                               float* s_score, int32_t* s_len, uint8_t* s_status, int* s_eligible) {
  const int g = blockIdx.x;
  const int tid = threadIdx.x;
  if (tid == 0) *s_eligible = 0;
  for (int c = tid; c < N; c += 256) {
    const int64_t r = (int64_t)c * G + g;
    s_key[c] = key[r];
    s_score[c] = score[r];
    const int len = length[r];
    s_len[c] = len < 0 ? 0 : (len > L ? L : len);                // (never read a row past its L ids, whatever length holds)
  }
  __syncthreads();

  int mine = 0;
  for (int c = tid; c < N; c += 256) {
    int st = candidate_status(c, g, G, L, s_key, s_score, s_len, packed, known_key, known_packed, known_len, M);
    if (known_dist && known_dist[(int64_t)c * G + g] < min_novelty) st |= MDT_SCREEN_KNOWN;
    if (reject) st |= reject[(int64_t)c * G + g];
    s_status[c] = (uint8_t)st;
    status[(int64_t)c * G + g] = (uint8_t)st;
    mine += st == 0;
  }
  if (mine) atomicAdd(s_eligible, mine);
  __syncthreads();
  return *s_eligible;
}

// One workgroup of 256 per group; the group's keys, scores, lengths and status bytes sit in LDS (17 KiB at N = 1024).
__global__ __launch_bounds__(256) void k_screen_select(const float* __restrict__ score, const uint64_t* __restrict__ key,
                                                       const int32_t* __restrict__ packed, const int32_t* __restrict__ length, int L,
                                                       int N, int G, const uint64_t* __restrict__ known_key,
                                                       const int32_t* __restrict__ known_packed,
                                                       const int32_t* __restrict__ known_len, int M, int K,
                                                       const uint8_t* __restrict__ reject, uint8_t* __restrict__ status,
                                                       int32_t* __restrict__ index, int32_t* __restrict__ count) {
  __shared__ uint64_t s_key[kScreenMaxN];
  __shared__ float s_score[kScreenMaxN];
  __shared__ int32_t s_len[kScreenMaxN];
  __shared__ uint8_t s_status[kScreenMaxN];
  __shared__ int s_eligible;
  const int g = blockIdx.x;
  const int tid = threadIdx.x;
  const int eligible = select_prologue(score, key, packed, length, L, N, G, known_key, known_packed, known_len, M, nullptr, 0, reject,
                                       status, s_key, s_score, s_len, s_status, &s_eligible);
  const int filled = eligible < K ? eligible : K;
  for (int c = tid; c < N; c += 256) {
    if (s_status[c]) continue;
    const float sc = s_score[c];
    int rank = 0;
    for (int o = 0; o < N; ++o)
      rank += s_status[o] == 0 && (s_score[o] < sc || (s_score[o] == sc && o < c));
    if (rank < K) index[(int64_t)g * K + rank] = c;
  }
  for (int k = filled + tid; k < K; k += 256) index[(int64_t)g * K + k] = -1;
  if (tid == 0) count[g] = filled;
}

// k_screen_select with two filters on the edit distance (mdt_device.h; rows of at most 64 ids below 64).  Status and order as
// above; then ONE pass over the eligible candidates in that order: a candidate closer than min_distance to a candidate kept before
// it is CLOSE, any other is kept while slots are left.  The pass runs to the end of the order, so the CLOSE bit of a candidate does
// not depend on where the slots ran out.  Inside a step the candidate is the pattern -- its 64 match masks in LDS, read by every
// thread at the same address -- and the threads share out the kept rows as texts; one block-wide "any closer".
// kFp (mdt_screen_select_similar): "closer" also when the candidate's fingerprint (fp (N*G,16), its popcount fp_count) is at least
// sim_num / 65536 Tanimoto-similar to a kept one's; the threads share out the kept rows in the same way, 16 words per pair.
// Without kFp the fingerprint arguments are not looked at and the code is the one that ran before the switch existed.
// kClass (mdt_screen_select_classes): "closer" also when the candidate's class_key is not 0 and at least max_per_class of the kept
// rows carry the same one; the threads share out the kept rows, and the count is block-wide: a wave reduction and one LDS word.
// Without kClass the class arguments are not looked at and the code is the one that ran before this switch existed.
template <bool kFp, bool kClass>
__global__ __launch_bounds__(256) void k_screen_select_diverse(
    const float* __restrict__ score, const uint64_t* __restrict__ key, const int32_t* __restrict__ packed,
    const int32_t* __restrict__ length, int L, int N, int G, const uint64_t* __restrict__ known_key,
    const int32_t* __restrict__ known_packed, const int32_t* __restrict__ known_len, int M, int K,
    const int32_t* __restrict__ known_dist, int min_novelty, int min_distance, const uint8_t* __restrict__ reject,
    const uint64_t* __restrict__ fp, const int32_t* __restrict__ fp_count, uint32_t sim_num,
    const uint64_t* __restrict__ class_key, int max_per_class, uint8_t* __restrict__ status, int32_t* __restrict__ index,
    int32_t* __restrict__ count) {
  __shared__ uint64_t s_key[kScreenMaxN];
  __shared__ float s_score[kScreenMaxN];
  __shared__ int32_t s_len[kScreenMaxN];
  __shared__ uint8_t s_status[kScreenMaxN];
  __shared__ int32_t s_order[kScreenMaxN];
  __shared__ int32_t s_kept[kScreenMaxN];
  __shared__ unsigned long long s_peq[64];
  __shared__ int s_eligible;
  __shared__ int s_same;
  const int g = blockIdx.x;
  const int tid = threadIdx.x;
  if constexpr (kClass)
    if (tid == 0) s_same = 0;                                    // (the prologue's barriers lie between this and its first use)
  const int eligible = select_prologue(score, key, packed, length, L, N, G, known_key, known_packed, known_len, M, known_dist,
                                       min_novelty, reject, status, s_key, s_score, s_len, s_status, &s_eligible);
  for (int c = tid; c < N; c += 256) {
    if (s_status[c]) continue;
    const float sc = s_score[c];
    int rank = 0;
    for (int o = 0; o < N; ++o)
      rank += s_status[o] == 0 && (s_score[o] < sc || (s_score[o] == sc && o < c));
    s_order[rank] = c;                                           // (the ranks of the eligible are 0 .. eligible - 1, each once)
  }
  __syncthreads();

  int kept = 0;                                                  // (the same in every thread)
  for (int e = 0; e < eligible; ++e) {
    const int c = s_order[e];
    const int m = s_len[c];                                      // >= 1: an empty row is not eligible
    int closer = 0;
    if constexpr (kClass) {
      __syncthreads();                                           // (s_kept and s_same as thread 0 left them in the step before)
      const uint64_t mine = class_key[(int64_t)c * G + g];       // (the same in every thread; class 0 is never counted)
      if (mine != 0) {
        int same = 0;
        for (int t = tid; t < kept; t += 256) same += class_key[(int64_t)s_kept[t] * G + g] == mine;
        for (int off = 32; off >= 1; off >>= 1) same += __shfl_xor(same, off, 64);
        if ((tid & 63) == 0 && same) atomicAdd(&s_same, same);
        __syncthreads();
        closer = s_same >= max_per_class;
      }
    }
    if constexpr (kFp) {
      __syncthreads();                                           // (s_kept as thread 0 left it in the step before)
      const uint64_t* mine = fp + ((int64_t)c * G + g) * 16;
      const int mine_count = fp_count[(int64_t)c * G + g];
      for (int t = tid; t < kept && !closer; t += 256) {
        const int64_t o = (int64_t)s_kept[t] * G + g;
        const uint64_t* other = fp + o * 16;
        int inter = 0;
        for (int w = 0; w < 16; ++w) inter += __popcll(mine[w] & other[w]);
        const int uni = mine_count + fp_count[o] - inter;
        closer = uni > 0 && (uint32_t)inter * (uint32_t)MDT_FP_SIM_DEN >= sim_num * (uint32_t)uni;
      }
    }
    if (min_distance > 1 && kept > 0) {
      const int32_t* row = packed + ((int64_t)c * G + g) * L;
      if (tid < 64) {                                            // the mask of symbol tid
        unsigned long long bits = 0;
        for (int j = 0; j < m; ++j) bits |= (unsigned long long)(row[j] == tid) << j;
        s_peq[tid] = bits;
      }
      __syncthreads();
      const unsigned long long top = edit_top(m);
      for (int t = tid; t < kept && !closer; t += 256) {      // (kFp: a thread that found a similar one skips this)
        const int o = s_kept[t];
        const int n = s_len[o];
        const int32_t* text = packed + ((int64_t)o * G + g) * L;
        unsigned long long pv = ~0ull, mv = 0;
        int d = m;
        for (int j = 0; j < n; ++j) {
          const int id = text[j];
          const unsigned long long eq = s_peq[id & 63];
          d += edit_step(edit_has_mask(id) ? eq : 0ull, top, pv, mv);
        }
        closer = d < min_distance;
      }
    }
    closer = __syncthreads_or(closer);                           // (also: s_peq and s_kept are free to be written again)
    if constexpr (kClass)
      if (tid == 0) s_same = 0;
    if (closer) {
      if (tid == 0) status[(int64_t)c * G + g] = MDT_SCREEN_CLOSE;
    } else if (kept < K) {
      if (tid == 0) {
        s_kept[kept] = c;
        index[(int64_t)g * K + kept] = c;
      }
      ++kept;
    }
  }
  for (int k = kept + tid; k < K; k += 256) index[(int64_t)g * K + k] = -1;
  if (tid == 0) count[g] = kept;
}

}  // namespace mdt

// ------------------------------------------------------------------------------------------------
// C ABI entry points of this translation unit (declared in include/mdt_hip.h)
// ------------------------------------------------------------------------------------------------
namespace {
// Every selection's checks and its launch.  name: what the messages start with; L_max: 1024 takes k_screen_select, 64 the diverse
// kernel (rows of one 64-bit word), which looks at the fingerprints iff with_fp and at the classes iff class_key is given (the
// entry point that takes them forwards a NULL class_key elsewhere, so here NULL means "not asked").  Two things here are as callers have come to know
// them, and the host tests pin both: the entry points with `reject` report under the name of the one without (they were added as
// its extension and share its messages), and with fingerprints the ranges are checked BEFORE an empty batch (G <= 0) returns 0,
// without them after.
int select_launch(const char* name, int L_max, bool with_fp, const float* score, const uint64_t* key, const int32_t* packed,
                  const int32_t* length, int32_t L, int32_t N, int32_t G, const uint64_t* known_key, const int32_t* known_packed,
                  const int32_t* known_len, int32_t M, int32_t K, const int32_t* known_dist, int32_t min_novelty,
                  int32_t min_distance, const uint8_t* reject, const uint64_t* fp, const int32_t* fp_count, int32_t sim_num,
                  const uint64_t* class_key, int32_t max_per_class, uint8_t* status, int32_t* index, int32_t* count, void* stream) {
  if (class_key && max_per_class < 1) return mdt_bad(name, ": need max_per_class >= 1");
  if (!with_fp && G <= 0) return 0;
  if (N < 1 || N > mdt::kScreenMaxN) return mdt_bad(name, ": need 1 <= N <= 1024 candidates per group");
  if (K < 1 || K > N) return mdt_bad(name, ": need 1 <= K <= N");
  if (L < 1 || L > L_max)
    return mdt_bad(name, L_max == 1024 ? ": need 1 <= L <= 1024"
                         : with_fp      ? ": need 1 <= L <= 64 positions per row"
                                        : ": need 1 <= L <= 64 (the edit distance takes rows of one 64-bit word)");
  if (M < 0) return mdt_bad(name, ": need M >= 0");
  if (with_fp && (sim_num < 1 || sim_num > MDT_FP_SIM_DEN)) return mdt_bad(name, ": need 1 <= sim_num <= 65536");
  if (G <= 0) return 0;
  if (M > 0 && (!known_key || !known_packed || !known_len))
    return mdt_bad(name, ": the known-set pointers may be NULL only when M == 0");
  if (!score || !key || !packed || !length || !status || !index || !count || (with_fp && (!fp || !fp_count)))
    return mdt_bad(name, ": null pointer");
  const dim3 grid((unsigned)G), block(256);
  if (L_max == 1024)
    hipLaunchKernelGGL(mdt::k_screen_select, grid, block, 0, (hipStream_t)stream, score, key, packed, length, L, N, G, known_key,
                       known_packed, known_len, M, K, reject, status, index, count);
  else if (class_key && with_fp)
    hipLaunchKernelGGL((mdt::k_screen_select_diverse<true, true>), grid, block, 0, (hipStream_t)stream, score, key, packed, length, L,
                       N, G, known_key, known_packed, known_len, M, K, known_dist, min_novelty, min_distance, reject, fp, fp_count,
                       (uint32_t)sim_num, class_key, max_per_class, status, index, count);
  else if (class_key)
    hipLaunchKernelGGL((mdt::k_screen_select_diverse<false, true>), grid, block, 0, (hipStream_t)stream, score, key, packed, length, L,
                       N, G, known_key, known_packed, known_len, M, K, known_dist, min_novelty, min_distance, reject,
                       (const uint64_t*)nullptr, (const int32_t*)nullptr, 0u, class_key, max_per_class, status, index, count);
  else if (with_fp)
    hipLaunchKernelGGL((mdt::k_screen_select_diverse<true, false>), grid, block, 0, (hipStream_t)stream, score, key, packed, length, L,
                       N, G, known_key, known_packed, known_len, M, K, known_dist, min_novelty, min_distance, reject, fp, fp_count,
                       (uint32_t)sim_num, (const uint64_t*)nullptr, 0, status, index, count);
  else
    hipLaunchKernelGGL((mdt::k_screen_select_diverse<false, false>), grid, block, 0, (hipStream_t)stream, score, key, packed, length,
                       L, N, G, known_key, known_packed, known_len, M, K, known_dist, min_novelty, min_distance, reject,
                       (const uint64_t*)nullptr, (const int32_t*)nullptr, 0u, (const uint64_t*)nullptr, 0, status, index, count);
  return mdt_finish(name);
}
}  // namespace

extern "C" {

int mdt_tokens_compact(const int32_t* tokens, int32_t B, int32_t L, float* fwd_in, int32_t Lf, double x_norm, int32_t* packed,
                       int32_t* length, uint64_t* key, void* stream) {
  if (B <= 0) return 0;
  if (!tokens || !packed || !length || !key) return mdt_bad("mdt_tokens_compact: null pointer");
  if (tokens == packed) return mdt_bad("mdt_tokens_compact: packed must not be the tokens themselves");
  if (L < 1) return mdt_bad("mdt_tokens_compact: need L >= 1");
  if (fwd_in && Lf < 1) return mdt_bad("mdt_tokens_compact: need Lf >= 1 with fwd_in");
  if (fwd_in && !(std::isfinite(x_norm) && x_norm != 0.0)) return mdt_bad("mdt_tokens_compact: x_norm must be finite and non-zero");
  hipLaunchKernelGGL(mdt::k_tokens_compact, dim3(((unsigned)B + 3) / 4), dim3(256), 0, (hipStream_t)stream, tokens, B, L, fwd_in,
                     Lf, x_norm, packed, length, key);
  return mdt_finish("mdt_tokens_compact");
}

int mdt_screen_score(const float* props, int64_t row_stride, const float* target, const float* weights, int32_t N, int32_t G,
                     int32_t n, float* score, void* stream) {
  if (N <= 0 || G <= 0) return 0;
  if (!props || !target || !score) return mdt_bad("mdt_screen_score: null pointer");
  if (n < 1 || n > 64) return mdt_bad("mdt_screen_score: need 1 <= n <= 64 properties");
  if (row_stride < n) return mdt_bad("mdt_screen_score: row_stride must be at least n");
  if ((int64_t)N * G > INT_MAX) return mdt_bad("mdt_screen_score: N * G exceeds 2^31 - 1 rows");
  const int rows = N * G;
  hipLaunchKernelGGL(mdt::k_screen_score, dim3(((unsigned)rows + 255) / 256), dim3(256), 0, (hipStream_t)stream, props, row_stride,
                     target, weights, rows, G, n, score);
  return mdt_finish("mdt_screen_score");
}

int mdt_screen_select_reject(const float* score, const uint64_t* key, const int32_t* packed, const int32_t* length, int32_t L,
                             int32_t N, int32_t G, const uint64_t* known_key, const int32_t* known_packed, const int32_t* known_len,
                             int32_t M, int32_t K, const uint8_t* reject, uint8_t* status, int32_t* index, int32_t* count,
                             void* stream) {
  return select_launch("mdt_screen_select", 1024, false, score, key, packed, length, L, N, G, known_key, known_packed, known_len, M,
                       K, nullptr, 0, 0, reject, nullptr, nullptr, 0, nullptr, 0, status, index, count, stream);
}

int mdt_screen_select(const float* score, const uint64_t* key, const int32_t* packed, const int32_t* length, int32_t L, int32_t N,
                      int32_t G, const uint64_t* known_key, const int32_t* known_packed, const int32_t* known_len, int32_t M,
                      int32_t K, uint8_t* status, int32_t* index, int32_t* count, void* stream) {
  return mdt_screen_select_reject(score, key, packed, length, L, N, G, known_key, known_packed, known_len, M, K, nullptr, status,
                                  index, count, stream);
}

int mdt_screen_select_diverse_reject(const float* score, const uint64_t* key, const int32_t* packed, const int32_t* length,
                                     int32_t L, int32_t N, int32_t G, const uint64_t* known_key, const int32_t* known_packed,
                                     const int32_t* known_len, int32_t M, int32_t K, const int32_t* known_dist, int32_t min_novelty,
                                     int32_t min_distance, const uint8_t* reject, uint8_t* status, int32_t* index, int32_t* count,
                                     void* stream) {
  return select_launch("mdt_screen_select_diverse", 64, false, score, key, packed, length, L, N, G, known_key, known_packed,
                       known_len, M, K, known_dist, min_novelty, min_distance, reject, nullptr, nullptr, 0, nullptr, 0, status, index,
                       count, stream);
}

int mdt_screen_select_similar(const float* score, const uint64_t* key, const int32_t* packed, const int32_t* length, int32_t L,
                              int32_t N, int32_t G, const uint64_t* known_key, const int32_t* known_packed, const int32_t* known_len,
                              int32_t M, int32_t K, const int32_t* known_dist, int32_t min_novelty, int32_t min_distance,
                              const uint8_t* reject, const uint64_t* fp, const int32_t* fp_count, int32_t sim_num, uint8_t* status,
                              int32_t* index, int32_t* count, void* stream) {
  if (!fp && !fp_count)                                         // no fingerprints: the selection as it was, the same launch
    return mdt_screen_select_diverse_reject(score, key, packed, length, L, N, G, known_key, known_packed, known_len, M, K,
                                            known_dist, min_novelty, min_distance, reject, status, index, count, stream);
  return select_launch("mdt_screen_select_similar", 64, true, score, key, packed, length, L, N, G, known_key, known_packed, known_len,
                       M, K, known_dist, min_novelty, min_distance, reject, fp, fp_count, sim_num, nullptr, 0, status, index, count,
                       stream);
}

int mdt_screen_select_classes(const float* score, const uint64_t* key, const int32_t* packed, const int32_t* length, int32_t L,
                              int32_t N, int32_t G, const uint64_t* known_key, const int32_t* known_packed, const int32_t* known_len,
                              int32_t M, int32_t K, const int32_t* known_dist, int32_t min_novelty, int32_t min_distance,
                              const uint8_t* reject, const uint64_t* fp, const int32_t* fp_count, int32_t sim_num,
                              const uint64_t* class_key, int32_t max_per_class, uint8_t* status, int32_t* index, int32_t* count,
                              void* stream) {
  if (!class_key)                                               // no classes: the selection as it was, the same launch
    return mdt_screen_select_similar(score, key, packed, length, L, N, G, known_key, known_packed, known_len, M, K, known_dist,
                                     min_novelty, min_distance, reject, fp, fp_count, sim_num, status, index, count, stream);
  return select_launch("mdt_screen_select_classes", 64, fp || fp_count, score, key, packed, length, L, N, G, known_key, known_packed,
                       known_len, M, K, known_dist, min_novelty, min_distance, reject, fp, fp_count, sim_num, class_key,
                       max_per_class, status, index, count, stream);
}

int mdt_screen_select_diverse(const float* score, const uint64_t* key, const int32_t* packed, const int32_t* length, int32_t L,
                              int32_t N, int32_t G, const uint64_t* known_key, const int32_t* known_packed, const int32_t* known_len,
                              int32_t M, int32_t K, const int32_t* known_dist, int32_t min_novelty, int32_t min_distance,
                              uint8_t* status, int32_t* index, int32_t* count, void* stream) {
  return mdt_screen_select_diverse_reject(score, key, packed, length, L, N, G, known_key, known_packed, known_len, M, K, known_dist,
                                          min_novelty, min_distance, nullptr, status, index, count, stream);
}

}  // extern "C"
