// Similarity of generated molecules on gfx950: a 1024-bit circular fingerprint of the molecular graph behind a row (the graph
// arrays of k_mol_graph, the neighbourhood hash of k_mol_key without a root) and the Tanimoto similarity of two fingerprints,
// |A & B| / |A | B|, as exact integer counts.
//
//   k_mol_fp       the graph arrays -> fp uint64 (R, 16) and its popcount; all zero for a row that is no molecule
//   k_fp_rows      inter[r], union[r] of row r of a against row r of b
//   k_fp_nearest   per query row the packed maximum (similarity quotient << 32 | ~known index) over one chunk of the known set
//   k_fp_finish    the packed maximum -> the known index, and inter and union of that pair, counted again
//
// The definition (degree, rounds, folding, thresholds, and what this is NOT: not RDKit's Morgan / ECFP) is written out at
// mdt_mol_fp in include/mdt_hip.h; the arithmetic is mdt_smiles_scan.h's fp_* functions, which a host program can run as well.
//
// k_mol_fp: one wave per row, LANE = ATOM, four rows (waves) per workgroup and no barrier across them.  The bond list is
// wave-uniform (scalar loads); the labels sit in LDS as [atom] words, so the neighbour's label is a broadcast read; every lane
// takes the bonds that touch it.  The 32 dwords of the fingerprint are built with LDS OR-atomics and written by 32 lanes.
//
// k_fp_nearest: grid (chunks of the known set, tiles of 64 queries), 4 waves, LANE = QUERY: the query's 32 dwords and its popcount
// stay in VGPRs, the known row is the same for the whole wave (a wave-uniform index through const __restrict__: scalar loads, scalar
// bit counts), so a pair costs 32 ANDs and 32 bit counts.  The best fraction of a lane is kept by cross-multiplied strict
// "greater" in ascending index order, so the lowest index survives a tie; no division inside the loop.
#include "mdt_kernels.h"
#include "mdt_device.h"
#include "mdt_smiles_scan.h"
#include "../../include/mdt_hip.h"

namespace mdt {

constexpr int kFpRowsPerBlock = 4;                             // k_mol_fp: waves (rows) of a workgroup
constexpr int kFpTile = 64;                                    // k_fp_nearest: query rows of a workgroup, one per lane
constexpr int kFpWaves = 4;                                    // ... its waves; each walks a quarter of the chunk
constexpr int kFpChunk = MDT_FP_KNOWN_CHUNK;                   // ... its known rows
static_assert(kFpChunk % kFpWaves == 0, "a wave takes a whole share of the chunk");
static_assert(kFpBits == MDT_FP_BITS && kFpSimDen == MDT_FP_SIM_DEN, "mdt_hip.h and mdt_smiles_scan.h agree");

__global__ __launch_bounds__(64 * kFpRowsPerBlock) void k_mol_fp(const int32_t* __restrict__ natoms,
                                                                 const uint32_t* __restrict__ atoms,
                                                                 const int32_t* __restrict__ nbonds,
                                                                 const uint32_t* __restrict__ bonds, int L, int R, int radius,
                                                                 uint64_t* __restrict__ fp, int32_t* __restrict__ count) {
  __shared__ uint64_t s_id[kFpRowsPerBlock][2][64];             // the labels of the round before and of this round
  __shared__ uint32_t s_fp[kFpRowsPerBlock][kFpDwords];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t row = (int64_t)blockIdx.x * kFpRowsPerBlock + wave;
  if (row >= R) return;                                         // (a whole wave leaves; nothing below crosses waves)
  uint32_t* out = reinterpret_cast<uint32_t*>(fp + row * kFpWords);      // dword d = bits 32 d .. 32 d + 31 (little-endian words)
  const int n = natoms[row], nb = nbonds[row];
  const uint32_t* row_bonds = bonds + row * L;
  if (!mol_graph_ok_wave(row_bonds, n, nb, L, lane)) {          // the rule of k_mol_key: such a row is no molecule
    if (lane < kFpDwords) out[lane] = 0;
    if (lane == 0) count[row] = 0;
    return;
  }
  if (lane < kFpDwords) s_fp[wave][lane] = 0;
  int deg = 0;
  for (int e = 0; e < nb; ++e) {
    const uint32_t w = row_bonds[e];
    deg += (int)(mol_a(w) == lane) + (int)(mol_b(w) == lane);
  }
  uint64_t id = lane < n ? fp_seed(atoms[row * L + lane], deg) : 0;
  wave_lds_sync();                                              // (s_fp is zero before the first bit is set)
  for (int r = 0;; ++r) {
    if (lane < n) {
      const int bit = fp_bit(id);
      atomicOr(&s_fp[wave][bit >> 5], 1u << (bit & 31));
    }
    if (r == radius) break;
    uint64_t* cur = s_id[wave][r & 1];
    cur[lane] = id;
    wave_lds_sync();
    uint64_t acc = 0;
    for (int e = 0; e < nb; ++e) {
      const uint32_t w = row_bonds[e];
      const int a = mol_a(w), b = mol_b(w);                                    // (< n <= 64: inside the labels)
      const uint64_t la = cur[a], lb = cur[b];                               // the same address in every lane
      const int times = (int)(a == lane) + (int)(b == lane);                 // (a bond of an atom to itself counts at both ends)
      const uint64_t term = fp_bond_term(a == lane ? lb : la, mol_order(w));
      acc += times == 2 ? 2 * term : (times ? term : 0);
    }
    id = fp_next(id, acc);
  }
  wave_lds_sync();
  int c = lane < kFpDwords ? __popc(s_fp[wave][lane]) : 0;
  if (lane < kFpDwords) out[lane] = s_fp[wave][lane];
  for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off, 64);
  if (lane == 0) count[row] = c;
}

__global__ __launch_bounds__(256) void k_fp_rows(const uint64_t* __restrict__ a, const uint64_t* __restrict__ b, int R,
                                                 int32_t* __restrict__ inter, int32_t* __restrict__ uni) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  int i, u;
  fp_counts(a + r * kFpWords, b + r * kFpWords, i, u);
  inter[r] = i;
  uni[r] = u;
}

// Wave w walks known rows chunk0 + w * (chunk / 4) ... in ascending order and keeps a strict maximum, so of equal fractions the
// lowest index stays; the waves' and the chunks' maxima are combined as one unsigned word (fp_pack), whose maximum is the same in
// any order.  A wave with nothing to walk contributes 0, which is below every word of a walked row.
__global__ __launch_bounds__(kFpTile* kFpWaves) void k_fp_nearest(const uint32_t* __restrict__ fp, int R,
                                                                  const uint32_t* __restrict__ known, int M,
                                                                  unsigned long long* __restrict__ best) {
  __shared__ unsigned long long s_part[kFpWaves][kFpTile];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t q = (int64_t)blockIdx.y * kFpTile + lane;
  uint32_t w[kFpDwords];
  int ca = 0;
#pragma unroll
  for (int i = 0; i < kFpDwords; ++i) {
    w[i] = q < R ? fp[q * kFpDwords + i] : 0u;
    ca += __popc(w[i]);
  }
  const int64_t chunk0 = (int64_t)blockIdx.x * kFpChunk;
  const int per_wave = kFpChunk / kFpWaves;
  const int64_t k0 = chunk0 + (int64_t)wave * per_wave;
  const int64_t k1 = k0 + per_wave < M ? k0 + per_wave : M;
  uint32_t best_i = 0, best_u = 1, best_k = (uint32_t)k0;        // similarity 0 at the first row of the share
  for (int64_t k = k0; k < k1; ++k) {
    const uint32_t* row = known + k * kFpDwords;                // wave-uniform
    int inter = 0, cb = 0;
#pragma unroll
    for (int i = 0; i < kFpDwords; ++i) {
      const uint32_t x = row[i];
      inter += __popc(w[i] & x);
      cb += __popc(x);
    }
    const uint32_t uni = (uint32_t)(ca + cb - inter);           // (0 only with inter == 0: never greater)
    if (fp_greater((uint32_t)inter, uni, best_i, best_u)) {
      best_i = (uint32_t)inter;
      best_u = uni;
      best_k = (uint32_t)k;
    }
  }
  s_part[wave][lane] = k0 < k1 ? fp_pack((int)best_i, (int)best_u, best_k) : 0ull;
  __syncthreads();
  if (wave == 0 && q < R) {
    unsigned long long mine = s_part[0][lane];
    for (int v = 1; v < kFpWaves; ++v) mine = s_part[v][lane] > mine ? s_part[v][lane] : mine;
    // the word only ever rises: a stale read costs an atomic that changes nothing, never a result
    if (mine > __atomic_load_n(best + q, __ATOMIC_RELAXED)) atomicMax(best + q, mine);
  }
}

__global__ __launch_bounds__(256) void k_fp_finish(const unsigned long long* __restrict__ best, const uint64_t* __restrict__ fp,
                                                   int R, const uint64_t* __restrict__ known, int M, int32_t* __restrict__ inter,
                                                   int32_t* __restrict__ uni, int32_t* __restrict__ index) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  uint32_t k = 0xFFFFFFFFu - (uint32_t)best[r];
  if (k >= (uint32_t)M) k = 0;                                  // (never: row 0 of the known set is always walked)
  int i, u;
  fp_counts(fp + r * kFpWords, known + (int64_t)k * kFpWords, i, u);
  inter[r] = i;
  uni[r] = u;
  index[r] = (int32_t)k;
}

}  // namespace mdt

// ------------------------------------------------------------------------------------------------
// C ABI entry points of this translation unit (declared in include/mdt_hip.h)
// ------------------------------------------------------------------------------------------------
extern "C" {

int mdt_mol_fp(const int32_t* natoms, const uint32_t* atoms, const int32_t* nbonds, const uint32_t* bonds, int32_t L, int32_t R,
               int32_t radius, uint64_t* fp, int32_t* count, void* stream) {
  if (R < 0) return mdt_bad("mdt_mol_fp: need R >= 0");
  if (L < 1 || L > mdt::kMolMaxL) return mdt_bad("mdt_mol_fp: need 1 <= L <= 64");
  if (radius < 0 || radius > mdt::kFpMaxRadius) return mdt_bad("mdt_mol_fp: need 0 <= radius <= 3");
  if (R == 0) return 0;
  if (!natoms || !atoms || !nbonds || !bonds || !fp || !count) return mdt_bad("mdt_mol_fp: null pointer");
  const unsigned blocks = (unsigned)(((int64_t)R + mdt::kFpRowsPerBlock - 1) / mdt::kFpRowsPerBlock);
  hipLaunchKernelGGL(mdt::k_mol_fp, dim3(blocks), dim3(64 * mdt::kFpRowsPerBlock), 0, (hipStream_t)stream, natoms, atoms, nbonds,
                     bonds, L, R, radius, fp, count);
  return mdt_finish("mdt_mol_fp");
}

int mdt_fp_tanimoto_rows(const uint64_t* a_fp, const uint64_t* b_fp, int32_t R, int32_t* inter, int32_t* uni, void* stream) {
  if (R < 0) return mdt_bad("mdt_fp_tanimoto_rows: need R >= 0");
  if (R == 0) return 0;
  if (!a_fp || !b_fp || !inter || !uni) return mdt_bad("mdt_fp_tanimoto_rows: null pointer");
  hipLaunchKernelGGL(mdt::k_fp_rows, dim3((unsigned)(((int64_t)R + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a_fp, b_fp, R,
                     inter, uni);
  return mdt_finish("mdt_fp_tanimoto_rows");
}

int mdt_fp_nearest(const uint64_t* fp, int32_t R, const uint64_t* known_fp, int32_t M, uint64_t* best, int32_t* inter, int32_t* uni,
                   int32_t* index, void* stream) {
  if (R < 0) return mdt_bad("mdt_fp_nearest: need R >= 0");
  if (M < 1) return mdt_bad("mdt_fp_nearest: need M >= 1 known rows");
  if (R == 0) return 0;
  if (!fp || !known_fp || !best || !inter || !uni || !index) return mdt_bad("mdt_fp_nearest: null pointer");
  const int64_t tiles = ((int64_t)R + mdt::kFpTile - 1) / mdt::kFpTile;
  if (tiles > 65535) return mdt_bad("mdt_fp_nearest: R exceeds 65535 * 64 rows");
  const unsigned chunks = (unsigned)(((int64_t)M + mdt::kFpChunk - 1) / mdt::kFpChunk);
  const unsigned blocks = (unsigned)(((int64_t)R + 255) / 256);
  unsigned long long* word = reinterpret_cast<unsigned long long*>(best);
  if (hipMemsetAsync(word, 0, (size_t)R * sizeof(unsigned long long), (hipStream_t)stream) != hipSuccess)
    return mdt_finish("mdt_fp_nearest");
  hipLaunchKernelGGL(mdt::k_fp_nearest, dim3(chunks, (unsigned)tiles), dim3(mdt::kFpTile * mdt::kFpWaves), 0, (hipStream_t)stream,
                     reinterpret_cast<const uint32_t*>(fp), R, reinterpret_cast<const uint32_t*>(known_fp), M, word);
  hipLaunchKernelGGL(mdt::k_fp_finish, dim3(blocks), dim3(256), 0, (hipStream_t)stream, word, fp, R, known_fp, M, inter, uni, index);
  return mdt_finish("mdt_fp_nearest");
}

}  // extern "C"
