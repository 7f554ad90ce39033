// Edit distance between molecules on gfx950: the global Levenshtein distance (insert, delete, substitute: 1 each) between
// compacted id rows (mdt_tokens_compact, k_screen.hip) of at most 64 ids below 64, by the bit-vector recurrence of mdt_device.h --
// one 64-bit word per pair, one pass over the text.
//
//   k_edit_rows      dist[r] = d(a[r], b[r]): one pair per lane, a wave of 64 pairs per workgroup
//   k_edit_nearest   per query row the packed minimum (distance << 32 | known index) over one chunk of the known set
//   k_edit_unpack    the packed minimum -> distance and index
//
// The match masks of the patterns sit in LDS as s_peq[symbol][lane]: in k_edit_nearest the text symbol is the same for the whole
// wave (every lane walks the same known row), so the 64 lanes read 64 consecutive words.  An id outside [0, 64) has no mask: it
// is skipped when the table is built and reads as 0 in the walk, so it matches nothing and never indexes the table.
#include "mdt_kernels.h"
#include "mdt_device.h"
#include "../../include/mdt_hip.h"

#include <climits>

namespace mdt {

constexpr int kEditTile = 64;                                  // query rows (patterns) of a workgroup: one per lane
constexpr int kEditWaves = 4;                                  // waves of a k_edit_nearest workgroup; they share the patterns
constexpr int kEditChunk = MDT_EDIT_KNOWN_CHUNK;               // known rows of a workgroup
static_assert(kEditChunk % kEditWaves == 0, "a wave takes a whole share of the chunk");

__device__ __forceinline__ int clamp_len(int len, int L) { return len < 0 ? 0 : (len > L ? L : len); }

// Column `lane` of the table from the pattern row[0:m].  The caller has zeroed the table and synchronised; a lane writes only
// its own column.
__device__ __forceinline__ void build_masks(unsigned long long* s_peq, int lane, const int32_t* row, int m) {
  for (int j = 0; j < m; ++j) {
    const int id = row[j];
    if (edit_has_mask(id)) s_peq[id * kEditTile + lane] |= 1ull << j;
  }
}

__global__ __launch_bounds__(kEditTile) void k_edit_rows(const int32_t* __restrict__ a, const int32_t* __restrict__ a_len,
                                                         const int32_t* __restrict__ b, const int32_t* __restrict__ b_len, int L,
                                                         int R, int32_t* __restrict__ dist) {
  __shared__ unsigned long long s_peq[64 * kEditTile];
  const int lane = threadIdx.x;
  const int64_t r = (int64_t)blockIdx.x * kEditTile + lane;
  for (int i = lane; i < 64 * kEditTile; i += kEditTile) s_peq[i] = 0;
  __syncthreads();
  if (r >= R) return;                                          // (no barrier below)
  const int m = clamp_len(a_len[r], L), n = clamp_len(b_len[r], L);
  build_masks(s_peq, lane, a + r * L, m);
  const int32_t* text = b + r * L;
  const unsigned long long top = edit_top(m);
  unsigned long long pv = ~0ull, mv = 0;
  int d = m;
  for (int j = 0; j < n; ++j) {
    const int id = text[j];
    const unsigned long long eq = s_peq[(id & 63) * kEditTile + lane];     // (always inside the table)
    d += edit_step(edit_has_mask(id) ? eq : 0ull, top, pv, mv);
  }
  dist[r] = m ? d : n;
}

// grid (chunks of the known set, tiles of 64 queries), 256 threads.  Wave w walks known rows chunk0 + w * 128 ... in ascending
// order and keeps a strict minimum, so of equal distances the lowest index stays; the waves' and the chunks' minima are combined
// as one unsigned word (distance << 32 | index), whose minimum is the same in any order.  A known row is skipped when the
// difference of the lengths -- a lower bound of the distance -- already reaches the current minimum of every lane (a wave vote:
// control flow stays uniform); such a row could only tie, and a tie at a higher index loses anyway.
__global__ __launch_bounds__(kEditTile* kEditWaves) void k_edit_nearest(const int32_t* __restrict__ packed,
                                                                        const int32_t* __restrict__ length, int L, int R,
                                                                        const int32_t* __restrict__ known_packed,
                                                                        const int32_t* __restrict__ known_len, int M,
                                                                        unsigned long long* __restrict__ best) {
  __shared__ unsigned long long s_peq[64 * kEditTile];
  __shared__ unsigned long long s_part[kEditWaves][kEditTile];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t q = (int64_t)blockIdx.y * kEditTile + lane;
  for (int i = tid; i < 64 * kEditTile; i += kEditTile * kEditWaves) s_peq[i] = 0;
  __syncthreads();
  const int m = q < R ? clamp_len(length[q], L) : 0;
  if (wave == 0 && q < R) build_masks(s_peq, lane, packed + q * L, m);
  __syncthreads();

  const unsigned long long top = edit_top(m);
  const int64_t chunk0 = (int64_t)blockIdx.x * kEditChunk;
  const int per_wave = kEditChunk / kEditWaves;
  const int64_t k0 = chunk0 + (int64_t)wave * per_wave;
  const int64_t k1 = k0 + per_wave < M ? k0 + per_wave : M;
  int best_d = INT_MAX;
  int best_i = 0;
  // A known row is read once, lane j its id j (one coalesced load, issued a row ahead); the walk takes id j out of lane j.
  int ahead = k0 < k1 && lane < L ? known_packed[k0 * L + lane] : 0;
  for (int64_t k = k0; k < k1; ++k) {
    const int ids = ahead;
    ahead = k + 1 < k1 && lane < L ? known_packed[(k + 1) * L + lane] : 0;
    const int n = clamp_len(known_len[k], L);
    const int gap = m > n ? m - n : n - m;
    if (__all(gap >= best_d)) continue;
    unsigned long long pv = ~0ull, mv = 0;
    int d = m;
    for (int j = 0; j < n; ++j) {
      const int id = __builtin_amdgcn_readlane(ids, j);
      const unsigned long long eq = s_peq[(id & 63) * kEditTile + lane];
      d += edit_step(edit_has_mask(id) ? eq : 0ull, top, pv, mv);
    }
    d = m ? d : n;
    if (d < best_d) {
      best_d = d;
      best_i = (int)k;
    }
  }
  s_part[wave][lane] = ((unsigned long long)(unsigned)best_d << 32) | (unsigned)best_i;     // (nothing walked: INT_MAX, above all)
  __syncthreads();
  if (wave == 0 && q < R) {
    unsigned long long mine = s_part[0][lane];
    for (int w = 1; w < kEditWaves; ++w) mine = s_part[w][lane] < mine ? s_part[w][lane] : mine;
    // the word only ever falls: a stale read costs an atomic that changes nothing, never a result
    if (mine < __atomic_load_n(best + q, __ATOMIC_RELAXED)) atomicMin(best + q, mine);
  }
}

__global__ __launch_bounds__(256) void k_edit_fill(unsigned long long* __restrict__ best, int R) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r < R) best[r] = ~0ull;
}

__global__ __launch_bounds__(256) void k_edit_unpack(const unsigned long long* __restrict__ best, int R, int32_t* __restrict__ dist,
                                                     int32_t* __restrict__ index) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  const unsigned long long w = best[r];
  dist[r] = (int32_t)(w >> 32);
  index[r] = (int32_t)(uint32_t)w;
}

}  // namespace mdt

// ------------------------------------------------------------------------------------------------
// C ABI entry points of this translation unit (declared in include/mdt_hip.h)
// ------------------------------------------------------------------------------------------------
extern "C" {

int mdt_edit_distance_rows(const int32_t* a_packed, const int32_t* a_len, const int32_t* b_packed, const int32_t* b_len, int32_t L,
                           int32_t R, int32_t* dist, void* stream) {
  if (R == 0) return 0;
  if (R < 0) return mdt_bad("mdt_edit_distance_rows: need R >= 0 rows");
  if (L < 1 || L > 64) return mdt_bad("mdt_edit_distance_rows: need 1 <= L <= 64 positions per row");
  if (!a_packed || !a_len || !b_packed || !b_len || !dist) return mdt_bad("mdt_edit_distance_rows: null pointer");
  const unsigned blocks = (unsigned)(((int64_t)R + mdt::kEditTile - 1) / mdt::kEditTile);
  hipLaunchKernelGGL(mdt::k_edit_rows, dim3(blocks), dim3(mdt::kEditTile), 0, (hipStream_t)stream, a_packed, a_len, b_packed, b_len,
                     L, R, dist);
  return mdt_finish("mdt_edit_distance_rows");
}

int mdt_edit_nearest(const int32_t* packed, const int32_t* length, int32_t L, int32_t R, const int32_t* known_packed,
                     const int32_t* known_len, int32_t M, uint64_t* best, int32_t* dist, int32_t* index, void* stream) {
  if (R == 0) return 0;
  if (R < 0) return mdt_bad("mdt_edit_nearest: need R >= 0 rows");
  if (L < 1 || L > 64) return mdt_bad("mdt_edit_nearest: need 1 <= L <= 64 positions per row");
  if (M < 1) return mdt_bad("mdt_edit_nearest: need M >= 1 known rows");
  if (!packed || !length || !known_packed || !known_len || !best || !dist || !index) return mdt_bad("mdt_edit_nearest: null pointer");
  const int64_t tiles = ((int64_t)R + mdt::kEditTile - 1) / mdt::kEditTile;
  if (tiles > 65535) return mdt_bad("mdt_edit_nearest: R exceeds 65535 * 64 rows");
  const unsigned chunks = (unsigned)(((int64_t)M + mdt::kEditChunk - 1) / mdt::kEditChunk);
  const unsigned blocks = (unsigned)(((int64_t)R + 255) / 256);
  unsigned long long* word = reinterpret_cast<unsigned long long*>(best);
  hipLaunchKernelGGL(mdt::k_edit_fill, dim3(blocks), dim3(256), 0, (hipStream_t)stream, word, R);
  hipLaunchKernelGGL(mdt::k_edit_nearest, dim3(chunks, (unsigned)tiles), dim3(mdt::kEditTile * mdt::kEditWaves), 0,
                     (hipStream_t)stream, packed, length, L, R, known_packed, known_len, M, word);
  hipLaunchKernelGGL(mdt::k_edit_unpack, dim3(blocks), dim3(256), 0, (hipStream_t)stream, word, R, dist, index);
  return mdt_finish("mdt_edit_nearest");
}

}  // extern "C"
