// Does the molecule contain this fragment?  Graph substructure match on gfx950: per (target row, pattern) whether an injective map
// of the pattern's atoms into the row's atoms keeps every atom and every bond of the pattern (subgraph monomorphism, on the graph
// arrays of k_mol_graph).  The definition -- the atom rule, the order of the depth-first search and its step cap, which is what
// makes "undecided" a defined answer -- is written out at mdt_sub_match in include/mdt_hip.h; the search itself is mdt_molsub.h's
// sub_root_search, which a host program runs as well.
//
// k_sub_match: 4 waves per workgroup, ONE WAVE PER TARGET ROW at a time (the waves walk the rows grid-stride), LANE t = TARGET ATOM t
// = SEARCH ROOT t.  Once per workgroup the P patterns are staged in LDS: their atoms, per atom the orders of its entries (p, p), and
// the other entries grouped by their later atom (e | order << 8 behind a start index per atom), so a lane at depth p walks the
// back-bonds of p and nothing else.  After that barrier the waves never meet again.  Per row (wave) in LDS: the five adj_o columns
// (64 words each, built by the lanes that own a bond with 64-bit OR), the compat words of the CURRENT pattern (one ballot per
// pattern atom; the loop over patterns is wave-uniform) and a found word.  Per lane: the map f, 36 bytes of LDS, lane-major -- 9
// dwords, odd, so equal depths of 32 lanes fall into 32 banks -- never a register array.  The candidate word of a depth is not
// stacked: on the way back it is computed again from f and masked to the bits above f[p].  28,944 B of LDS per workgroup (8,448 B
// of patterns, 5,124 B a wave), 0 bytes of scratch.
#include "mdt_kernels.h"
#include "mdt_device.h"
#include "mdt_molsub.h"
#include "../../include/mdt_hip.h"

namespace mdt {

constexpr int kSubRowsPerBlock = 4;                            // waves of a workgroup, one target row each at a time
constexpr int kSubFStride = 36;                                // bytes of one lane's map: kSubMaxWidth and one more dword
constexpr int kSubMaxBlocks = 2048;                            // 8 workgroups for each of 256 compute units
static_assert(kSubMaxPatterns == MDT_SUB_MAX_PATTERNS && kSubMaxWidth == MDT_SUB_MAX_WIDTH && kSubMaxSteps == MDT_SUB_MAX_STEPS,
              "mdt_hip.h and mdt_molsub.h agree");
static_assert(kSubFStride >= kSubMaxWidth && (kSubFStride / 4) % 2 == 1, "a map fits and its stride is an odd number of dwords");

// "another root of this row has succeeded": the only reason for which a root may stop early
struct SubWaveSignal {
  uint32_t* word;
  __device__ __forceinline__ bool stop() const { return __atomic_load_n(word, __ATOMIC_RELAXED) != 0; }
  __device__ __forceinline__ void found() const { __atomic_store_n(word, 1u, __ATOMIC_RELAXED); }
};

__device__ __forceinline__ int sub_key(uint32_t w) {            // the later atom of an entry; 255 for an entry (p, p)
  const int a = mol_a(w), b = mol_b(w);
  return a == b ? 255 : (a > b ? a : b);
}

__global__ __launch_bounds__(64 * kSubRowsPerBlock) void k_sub_match(
    const int32_t* __restrict__ natoms, const uint32_t* __restrict__ atoms, const int32_t* __restrict__ nbonds,
    const uint32_t* __restrict__ bonds, int L, int R, const int32_t* __restrict__ p_natoms, const uint32_t* __restrict__ p_atoms,
    const int32_t* __restrict__ p_nbonds, const uint32_t* __restrict__ p_bonds, int LP, int P, uint32_t need, uint32_t ban,
    uint32_t* __restrict__ match, uint32_t* __restrict__ undecided, uint8_t* __restrict__ flags) {
  __shared__ uint32_t s_patom[kSubMaxPatterns][kSubMaxWidth];
  __shared__ uint16_t s_back[kSubMaxPatterns][kSubMaxWidth];
  __shared__ uint8_t s_bstart[kSubMaxPatterns][kSubFStride];    // [p] .. [p + 1]: the back-bonds of p; m + 1 <= 33 entries
  __shared__ uint8_t s_selfneed[kSubMaxPatterns][kSubMaxWidth];
  __shared__ int32_t s_pm[kSubMaxPatterns];                     // the pattern's atoms, 0: it matches nothing
  __shared__ unsigned long long s_adj[kSubRowsPerBlock][kSubOrders * 64];
  __shared__ uint64_t s_compat[kSubRowsPerBlock][kSubMaxWidth];
  __shared__ uint8_t s_f[kSubRowsPerBlock][64 * kSubFStride];
  __shared__ uint32_t s_found[kSubRowsPerBlock];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

  // ---- the patterns, once per workgroup: wave w takes patterns w, w + 4, ... (q < P <= 32) ----
  for (int q = wave; q < P; q += kSubRowsPerBlock) {
    const int m = p_natoms[q], mb = p_nbonds[q];
    const uint32_t* q_bonds = p_bonds + q * LP;
    bool ok = mol_counts_ok(m, mb, LP);
    const bool mine = ok && lane < mb;                          // (mb <= LP <= 32 lanes own an entry)
    const uint32_t w = mine ? q_bonds[lane] : 0u;
    ok = ok && !__any(mine && (mol_a(w) >= m || mol_b(w) >= m || !mol_order_ok(mol_order(w))));
    if (lane == 0) s_pm[q] = ok ? m : 0;
    if (!ok) continue;                                          // (wave-uniform)
    if (lane < m) s_patom[q][lane] = p_atoms[q * LP + lane];
    const int key = sub_key(w);
    int pos = 0, start = 0, self = 0;
    for (int k = 0; k < mb; ++k) {                              // bounded by mb <= LP; entry k is the same in every lane
      const uint32_t wk = q_bonds[k];
      const int kk = sub_key(wk);
      pos += (int)(kk < key || (kk == key && k < lane));        // entries sorted by later atom, then by index
      start += (int)(kk < lane);                                // lane as pattern atom: the entries of the atoms before it
      if (kk == 255 && mol_a(wk) == lane) self |= 1 << (mol_order(wk) - 1);
    }
    if (mine && key != 255)                                     // (pos < the entries that are no (p, p): inside the row)
      s_back[q][pos] = (uint16_t)((mol_a(w) < mol_b(w) ? mol_a(w) : mol_b(w)) | mol_order(w) << 8);
    if (lane <= m) s_bstart[q][lane] = (uint8_t)start;          // (m <= 32 < kSubFStride)
    if (lane < m) s_selfneed[q][lane] = (uint8_t)self;
  }
  __syncthreads();

  unsigned long long* adj = s_adj[wave];
  uint64_t* compat = s_compat[wave];
  const SubWaveSignal signal{&s_found[wave]};
  // ---- the rows: bounded by R ----
  for (int64_t row = (int64_t)blockIdx.x * kSubRowsPerBlock + wave; row < R; row += (int64_t)gridDim.x * kSubRowsPerBlock) {
    const int n = natoms[row], nb = nbonds[row];
    bool ok = mol_counts_ok(n, nb, L);                          // the rule of k_mol_key: such a row is no molecule
    const bool mine = ok && lane < nb;                          // (nb <= L <= 64 lanes own an entry)
    const uint32_t w = mine ? bonds[row * L + lane] : 0u;
    ok = ok && !__any(mine && (mol_a(w) >= n || mol_b(w) >= n));
    uint32_t mt = 0, und = 0;
    if (ok) {
      for (int o = 0; o < kSubOrders; ++o) adj[o * 64 + lane] = 0;
      wave_lds_sync();
      if (mine && mol_order_ok(mol_order(w))) {                 // (a, b < n <= 64, order in 1..5: inside the five columns)
        atomicOr(&adj[(mol_order(w) - 1) * 64 + mol_a(w)], 1ull << mol_b(w));
        atomicOr(&adj[(mol_order(w) - 1) * 64 + mol_b(w)], 1ull << mol_a(w));
      }
      wave_lds_sync();
      const uint32_t desc = lane < n ? atoms[row * L + lane] : 0u;
      uint32_t have = 0;                                        // the orders of this atom's entries (t, t)
      for (int o = 0; o < kSubOrders; ++o) have |= (uint32_t)((adj[o * 64 + lane] >> lane) & 1ull) << o;
      for (int q = 0; q < P; ++q) {                             // wave-uniform, bounded by P <= 32
        const int m = __builtin_amdgcn_readfirstlane(s_pm[q]);
        if (m == 0 || m > n) continue;
        bool empty = false;
        uint64_t roots = 0;
        for (int p = 0; p < m; ++p) {                           // bounded by m <= LP
          const bool acc = lane < n && sub_accepts(s_patom[q][p], desc) && (s_selfneed[q][p] & ~have) == 0;
          const uint64_t word = __ballot(acc);
          if (lane == 0) compat[p] = word;
          if (p == 0) roots = word;
          empty = empty || word == 0;
        }
        if (empty) continue;
        if (m == 1) {
          mt |= 1u << q;
          continue;
        }
        if (lane == 0) s_found[wave] = 0;
        wave_lds_sync();
        int code = kSubNone;
        if ((roots >> lane) & 1ull) {
          // every loop inside is bounded by the back-bonds of one atom (<= LP) or by the step cap (see sub_root_search)
          const SubTables t{compat, (const uint64_t*)adj, s_bstart[q], s_back[q], s_f[wave] + lane * kSubFStride, 1};
          int steps;
          code = sub_root_search(t, m, lane, steps, signal);
        }
        const bool found = __any(code == kSubFound), capped = __any(code == kSubCapped);
        if (found) mt |= 1u << q;
        else if (capped) und |= 1u << q;
        wave_lds_sync();                                        // (the next pattern writes compat and the found word again)
      }
    }
    if (lane == 0) {
      match[row] = mt;
      undecided[row] = und;
      if (flags) flags[row] = ((mt & need) != need || ((mt | und) & ban) != 0) ? (uint8_t)MDT_SCREEN_SUBSTRUCTURE : (uint8_t)0;
    }
  }
}

// Which atoms match, and how often (mdt_sub_map in include/mdt_hip.h).  k_sub_match's layout -- 4 waves, one wave per row at a time,
// lane = target atom = root, the patterns staged once per workgroup, adj / compat / f in LDS -- with sub_root_enumerate in place of
// the first-success search: every root runs to the end of its tree or to the cap, so there is no found word and no early stop.
// Per lane in registers: the union of its images (one 64-bit OR an embedding) and its embedding count; per wave in LDS one 64-bit
// cover word (atomic OR, once per root that saw a map) and one 32-bit sum.  The first map of the lowest found root is not kept
// while enumerating: after the ballot that ONE lane runs sub_root_search again into its own f (at most kSubMaxSteps steps, the
// walk up to its first success), and lanes p < LP read it from there.  That costs no LDS; a second per-lane map would cost 9,216 B
// a workgroup.  The staging is k_sub_match's, spelled out again: that kernel is left as it was, instruction for instruction.
// 28,976 B of LDS per workgroup, 0 bytes of scratch.  Every output word is written here, by plain vector stores.
__global__ __launch_bounds__(64 * kSubRowsPerBlock) void k_sub_map(
    const int32_t* __restrict__ natoms, const uint32_t* __restrict__ atoms, const int32_t* __restrict__ nbonds,
    const uint32_t* __restrict__ bonds, int L, int R, const int32_t* __restrict__ p_natoms, const uint32_t* __restrict__ p_atoms,
    const int32_t* __restrict__ p_nbonds, const uint32_t* __restrict__ p_bonds, int LP, int P, const uint8_t* __restrict__ count_lo,
    const uint8_t* __restrict__ count_hi, unsigned long long* __restrict__ found, unsigned long long* __restrict__ capped,
    uint32_t* __restrict__ embeddings, unsigned long long* __restrict__ cover, uint8_t* __restrict__ map, uint8_t* __restrict__ flags) {
  __shared__ uint32_t s_patom[kSubMaxPatterns][kSubMaxWidth];
  __shared__ uint16_t s_back[kSubMaxPatterns][kSubMaxWidth];
  __shared__ uint8_t s_bstart[kSubMaxPatterns][kSubFStride];    // [p] .. [p + 1]: the back-bonds of p; m + 1 <= 33 entries
  __shared__ uint8_t s_selfneed[kSubMaxPatterns][kSubMaxWidth];
  __shared__ int32_t s_pm[kSubMaxPatterns];                     // the pattern's atoms, 0: it matches nothing
  __shared__ unsigned long long s_adj[kSubRowsPerBlock][kSubOrders * 64];
  __shared__ uint64_t s_compat[kSubRowsPerBlock][kSubMaxWidth];
  __shared__ uint8_t s_f[kSubRowsPerBlock][64 * kSubFStride];
  __shared__ unsigned long long s_cover[kSubRowsPerBlock];
  __shared__ uint32_t s_sum[kSubRowsPerBlock];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

  // ---- the patterns, once per workgroup: wave w takes patterns w, w + 4, ... (q < P <= 32) ----
  for (int q = wave; q < P; q += kSubRowsPerBlock) {            // bounded by P
    const int m = p_natoms[q], mb = p_nbonds[q];
    const uint32_t* q_bonds = p_bonds + q * LP;
    bool ok = mol_counts_ok(m, mb, LP);
    const bool mine = ok && lane < mb;                          // (mb <= LP <= 32 lanes own an entry)
    const uint32_t w = mine ? q_bonds[lane] : 0u;
    ok = ok && !__any(mine && (mol_a(w) >= m || mol_b(w) >= m || !mol_order_ok(mol_order(w))));
    if (lane == 0) s_pm[q] = ok ? m : 0;
    if (!ok) continue;                                          // (wave-uniform)
    if (lane < m) s_patom[q][lane] = p_atoms[q * LP + lane];
    const int key = sub_key(w);
    int pos = 0, start = 0, self = 0;
    for (int k = 0; k < mb; ++k) {                              // bounded by mb <= LP; entry k is the same in every lane
      const uint32_t wk = q_bonds[k];
      const int kk = sub_key(wk);
      pos += (int)(kk < key || (kk == key && k < lane));        // entries sorted by later atom, then by index
      start += (int)(kk < lane);                                // lane as pattern atom: the entries of the atoms before it
      if (kk == 255 && mol_a(wk) == lane) self |= 1 << (mol_order(wk) - 1);
    }
    if (mine && key != 255)                                     // (pos < the entries that are no (p, p): inside the row)
      s_back[q][pos] = (uint16_t)((mol_a(w) < mol_b(w) ? mol_a(w) : mol_b(w)) | mol_order(w) << 8);
    if (lane <= m) s_bstart[q][lane] = (uint8_t)start;          // (m <= 32 < kSubFStride)
    if (lane < m) s_selfneed[q][lane] = (uint8_t)self;
  }
  __syncthreads();

  unsigned long long* adj = s_adj[wave];
  uint64_t* compat = s_compat[wave];
  uint8_t* my_f = s_f[wave] + lane * kSubFStride;
  // ---- the rows: bounded by R ----
  for (int64_t row = (int64_t)blockIdx.x * kSubRowsPerBlock + wave; row < R; row += (int64_t)gridDim.x * kSubRowsPerBlock) {
    const int n = natoms[row], nb = nbonds[row];
    bool ok = mol_counts_ok(n, nb, L);                          // the rule of k_mol_key: such a row is no molecule
    const bool mine = ok && lane < nb;                          // (nb <= L <= 64 lanes own an entry)
    const uint32_t w = mine ? bonds[row * L + lane] : 0u;
    ok = ok && !__any(mine && (mol_a(w) >= n || mol_b(w) >= n));
    uint32_t desc = 0, have = 0;
    if (ok) {
      for (int o = 0; o < kSubOrders; ++o) adj[o * 64 + lane] = 0;   // bounded by the five orders
      wave_lds_sync();
      if (mine && mol_order_ok(mol_order(w))) {                 // (a, b < n <= 64, order in 1..5: inside the five columns)
        atomicOr(&adj[(mol_order(w) - 1) * 64 + mol_a(w)], 1ull << mol_b(w));
        atomicOr(&adj[(mol_order(w) - 1) * 64 + mol_b(w)], 1ull << mol_a(w));
      }
      wave_lds_sync();
      desc = lane < n ? atoms[row * L + lane] : 0u;
      for (int o = 0; o < kSubOrders; ++o) have |= (uint32_t)((adj[o * 64 + lane] >> lane) & 1ull) << o;   // the entries (t, t)
    }
    bool outside = false;
    for (int q = 0; q < P; ++q) {                               // wave-uniform, bounded by P <= 32
      const int m = ok ? __builtin_amdgcn_readfirstlane(s_pm[q]) : 0;
      uint64_t fnd = 0, cap = 0, cov = 0;
      uint32_t emb = 0;
      int image = 0;                                            // this lane's byte of the map: 1 + f(lane), 0 for none
      bool search = m != 0 && m <= n;
      uint64_t roots = 0;
      if (search) {
        bool empty = false;
        for (int p = 0; p < m; ++p) {                           // bounded by m <= LP
          const bool acc = lane < n && sub_accepts(s_patom[q][p], desc) && (s_selfneed[q][p] & ~have) == 0;
          const uint64_t word = __ballot(acc);
          if (lane == 0) compat[p] = word;
          if (p == 0) roots = word;
          empty = empty || word == 0;
        }
        search = !empty;
      }
      if (search && m == 1) {                                   // every accepted atom is an anchor, a map and its own image
        fnd = cov = roots;
        emb = (uint32_t)mol_popc(roots);
        image = lane == 0 ? 1 + mol_lowest(roots) : 0;
      } else if (search) {
        if (lane == 0) s_cover[wave] = 0, s_sum[wave] = 0;
        wave_lds_sync();
        // every loop inside is bounded by the back-bonds of one atom (<= LP) or by the step cap (see sub_root_enumerate)
        const SubTables t{compat, (const uint64_t*)adj, s_bstart[q], s_back[q], my_f, 1};
        uint32_t seen = 0;
        bool cut = false;
        if ((roots >> lane) & 1ull) {
          int steps;
          SubCoverSink sink{0};
          seen = sub_root_enumerate(t, m, lane, steps, cut, sink);
          if (seen) {
            atomicOr(&s_cover[wave], (unsigned long long)sink.cover);
            atomicAdd(&s_sum[wave], seen);                      // (at most 64 roots of kSubMaxSteps maps: no overflow)
          }
        }
        fnd = __ballot(seen != 0);
        cap = __ballot(cut);
        const int low = fnd ? mol_lowest(fnd) : -1;             // (wave-uniform)
        if (lane == low) {                                      // the first map of the lowest found root: its walk once more
          int steps;
          SubNoSignal alone;
          sub_root_search(t, m, lane, steps, alone);            // bounded by the step cap; it succeeds, as the enumeration did
        }
        wave_lds_sync();
        cov = s_cover[wave];
        emb = s_sum[wave];
        if (low >= 0 && lane < m) image = 1 + s_f[wave][low * kSubFStride + lane];   // (lane < m <= 32 = a map's bytes)
      }
      const int64_t pair = row * P + q;
      if (lane == 0) {
        found[pair] = fnd;
        capped[pair] = cap;
        embeddings[pair] = emb;
        cover[pair] = cov;
      }
      if (lane < LP) map[pair * LP + lane] = (uint8_t)image;    // (LP <= 32 lanes own a byte)
      if (count_lo) outside = outside || sub_count_outside(fnd, cap, count_lo[q], count_hi[q]);
      wave_lds_sync();                                          // (the next pattern writes compat, f and the two words again)
    }
    if (flags && lane == 0) flags[row] = outside ? (uint8_t)MDT_SCREEN_SUBSTRUCTURE : (uint8_t)0;
  }
}

}  // namespace mdt

// ------------------------------------------------------------------------------------------------
// C ABI entry point of this translation unit (declared in include/mdt_hip.h)
// ------------------------------------------------------------------------------------------------
extern "C" int mdt_sub_match(const int32_t* natoms, const uint32_t* atoms, const int32_t* nbonds, const uint32_t* bonds, int32_t L,
                             int32_t R, const int32_t* p_natoms, const uint32_t* p_atoms, const int32_t* p_nbonds,
                             const uint32_t* p_bonds, int32_t LP, int32_t P, uint32_t need, uint32_t ban, uint32_t* match,
                             uint32_t* undecided, uint8_t* flags, void* stream) {
  if (R < 0) return mdt_bad("mdt_sub_match: need R >= 0");
  if (L < 1 || L > mdt::kMolMaxL) return mdt_bad("mdt_sub_match: need 1 <= L <= 64");
  if (LP < 1 || LP > mdt::kSubMaxWidth) return mdt_bad("mdt_sub_match: need 1 <= LP <= 32");
  if (P < 1 || P > mdt::kSubMaxPatterns) return mdt_bad("mdt_sub_match: need 1 <= P <= 32");
  const uint32_t all = P == 32 ? 0xFFFFFFFFu : (1u << P) - 1u;
  if ((need | ban) & ~all) return mdt_bad("mdt_sub_match: need and ban may only have bits below P");
  if (need & ban) return mdt_bad("mdt_sub_match: need and ban may not overlap");
  if (R == 0) return 0;
  if (!natoms || !atoms || !nbonds || !bonds || !p_natoms || !p_atoms || !p_nbonds || !p_bonds || !match || !undecided)
    return mdt_bad("mdt_sub_match: null pointer");
  const int64_t want = ((int64_t)R + mdt::kSubRowsPerBlock - 1) / mdt::kSubRowsPerBlock;
  const unsigned blocks = (unsigned)(want < mdt::kSubMaxBlocks ? want : mdt::kSubMaxBlocks);
  hipLaunchKernelGGL(mdt::k_sub_match, dim3(blocks), dim3(64 * mdt::kSubRowsPerBlock), 0, (hipStream_t)stream, natoms, atoms, nbonds,
                     bonds, L, R, p_natoms, p_atoms, p_nbonds, p_bonds, LP, P, need, ban, match, undecided, flags);
  return mdt_finish("mdt_sub_match");
}

extern "C" int mdt_sub_map(const int32_t* natoms, const uint32_t* atoms, const int32_t* nbonds, const uint32_t* bonds, int32_t L,
                           int32_t R, const int32_t* p_natoms, const uint32_t* p_atoms, const int32_t* p_nbonds,
                           const uint32_t* p_bonds, int32_t LP, int32_t P, const uint8_t* count_lo, const uint8_t* count_hi,
                           uint64_t* found, uint64_t* capped, uint32_t* embeddings, uint64_t* cover, uint8_t* map, uint8_t* flags,
                           void* stream) {
  if (R < 0) return mdt_bad("mdt_sub_map: need R >= 0");
  if (L < 1 || L > mdt::kMolMaxL) return mdt_bad("mdt_sub_map: need 1 <= L <= 64");
  if (LP < 1 || LP > mdt::kSubMaxWidth) return mdt_bad("mdt_sub_map: need 1 <= LP <= 32");
  if (P < 1 || P > mdt::kSubMaxPatterns) return mdt_bad("mdt_sub_map: need 1 <= P <= 32");
  if ((count_lo == nullptr) != (count_hi == nullptr)) return mdt_bad("mdt_sub_map: count_lo and count_hi must be both NULL or both given");
  if (flags && !count_lo) return mdt_bad("mdt_sub_map: flags needs count_lo and count_hi");
  if (R == 0) return 0;
  if (!natoms || !atoms || !nbonds || !bonds || !p_natoms || !p_atoms || !p_nbonds || !p_bonds || !found || !capped || !embeddings ||
      !cover || !map)
    return mdt_bad("mdt_sub_map: null pointer");
  const int64_t want = ((int64_t)R + mdt::kSubRowsPerBlock - 1) / mdt::kSubRowsPerBlock;
  const unsigned blocks = (unsigned)(want < mdt::kSubMaxBlocks ? want : mdt::kSubMaxBlocks);
  hipLaunchKernelGGL(mdt::k_sub_map, dim3(blocks), dim3(64 * mdt::kSubRowsPerBlock), 0, (hipStream_t)stream, natoms, atoms, nbonds,
                     bonds, L, R, p_natoms, p_atoms, p_nbonds, p_bonds, LP, P, count_lo, count_hi, (unsigned long long*)found,
                     (unsigned long long*)capped, embeddings, (unsigned long long*)cover, map, flags);
  return mdt_finish("mdt_sub_map");
}
