// Graph substructure match (mdt_hip.h, mdt_sub_match): the atom rule and the depth-first search of one root with its step count;
// the bond word and the check made before any search (mol_graph_ok) are mdt_smiles_scan.h's.  Like that header everything here is
// __host__ __device__ and touches only the arrays it is handed, so the kernel (k_molsub.hip: tables in LDS, one root per lane) and
// a host program (tools/molsub_host_check.cpp: tables in arrays of exactly their size) run the same search.
#pragma once

#include <cstdint>
#include <hip/hip_runtime.h>

#include "mdt_smiles_scan.h"

namespace mdt {

constexpr int kSubMaxPatterns = 32, kSubMaxWidth = 32, kSubMaxSteps = 4096, kSubOrders = kMolOrders;
enum { kSubNone = 0, kSubFound = 1, kSubCapped = 2, kSubStopped = 3 };   // what one root's search ends with

// which bits of the descriptor pattern atom p compares: symbol and aromatic bit unless it is '*', charge, H count and isotope when it
// is bracketed; the bracket bit itself never
__host__ __device__ __forceinline__ uint32_t sub_atom_mask(uint32_t p) {
  return ((p & kMolBracket) ? 0xFFFFF000u : 0u) | ((p & 31u) == (uint32_t)kMolStar ? 0u : 0x7FFu);
}
__host__ __device__ __forceinline__ bool sub_accepts(uint32_t p, uint32_t t) { return ((p ^ t) & sub_atom_mask(p)) == 0; }
// the bits above bit t
__host__ __device__ __forceinline__ uint64_t sub_above(int t) { return ~(((uint64_t)2 << t) - 1); }
__host__ __device__ __forceinline__ int sub_lowest(uint64_t w) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __ffsll((unsigned long long)w) - 1;
#else
  return __builtin_ctzll(w);
#endif
}

// The tables of one (target row, pattern) pair, wherever they live.
//   compat[p]                   the target atoms that pattern atom p accepts, p < m
//   adj[(o - 1) * 64 + u]       the atoms joined to target atom u by an entry of order o, 1 <= o <= 5
//   back_start[p], back[k]      the back-bonds of p are back[back_start[p] .. back_start[p + 1]), each e | o << 8 with e < p
//   f[p * f_stride]             the map of THIS root, m entries
struct SubTables {
  const uint64_t* compat;
  const uint64_t* adj;
  const uint8_t* back_start;
  const uint16_t* back;
  uint8_t* f;
  int f_stride;
};

// the candidates of pattern atom p under the partial map f[0 .. p): bounded by the back-bonds of p, at most kSubMaxWidth
__host__ __device__ __forceinline__ uint64_t sub_candidates(const SubTables& t, int p, uint64_t used) {
  uint64_t c = t.compat[p] & ~used;
  const int k1 = t.back_start[p + 1];
  for (int k = t.back_start[p]; k < k1; ++k) {
    const uint32_t w = t.back[k];
    c &= t.adj[((int)(w >> 8) - 1) * 64 + t.f[(int)(w & 255u) * t.f_stride]];
  }
  return c;
}

// The search of one root (2 <= m <= n, root in compat[0]): f(0) = root, pattern atoms in index order, candidates in ascending target
// index.  -> kSubFound when atom m - 1 is assigned, kSubNone when the root is exhausted, kSubCapped when step kSubMaxSteps + 1 would
// be made, kSubStopped when signal.stop() said that another root has succeeded (signal.found() is told of this one's success);
// steps: the assignments f(p) = t, p >= 1, made.  Every pass of the loop makes a step or takes one back, so it runs at most
// 2 * kSubMaxSteps + 2 times.
template <class Signal>
__host__ __device__ inline int sub_root_search(const SubTables& t, int m, int root, int& steps, Signal& signal) {
  t.f[0] = (uint8_t)root;
  uint64_t used = (uint64_t)1 << root;
  int p = 1, made = 0, code;
  uint64_t cand = sub_candidates(t, 1, used);
  for (;;) {                                                    // bounded: at most kSubMaxSteps steps, and as many taken back
    if (signal.stop()) { code = kSubStopped; break; }
    if (cand == 0) {                                            // back: the next candidate of the atom before, above its last one
      --p;
      if (p == 0) { code = kSubNone; break; }
      const int last = t.f[p * t.f_stride];
      used &= ~((uint64_t)1 << last);
      cand = sub_candidates(t, p, used) & sub_above(last);
      continue;
    }
    if (made == kSubMaxSteps) { code = kSubCapped; break; }
    const int at = sub_lowest(cand);
    t.f[p * t.f_stride] = (uint8_t)at;
    ++made;
    if (p == m - 1) { signal.found(); code = kSubFound; break; }
    used |= (uint64_t)1 << at;
    ++p;
    cand = sub_candidates(t, p, used);
  }
  steps = made;
  return code;
}

// the signal of a search that runs alone
struct SubNoSignal {
  __host__ __device__ __forceinline__ bool stop() const { return false; }
  __host__ __device__ __forceinline__ void found() const {}
};

// One (row, pattern) pair, root after root, in the order the definition is written down: -> kSubFound (match), kSubCapped
// (undecided) or kSubNone.  root_code[0:n] / root_steps[0:n], when given, take every root's own end and step count (-1 / 0 for a
// target atom that is no root); no root stops for another.  Reads atoms[0:n], bonds[0:nb], p_atoms[0:m], p_bonds[0:mb] and nothing
// beyond.  k_sub_match computes the same with one root per lane and the tables in LDS.
__host__ __device__ inline int sub_match_pair(const uint32_t* atoms, const uint32_t* bonds, int n, int nb, int L,
                                              const uint32_t* p_atoms, const uint32_t* p_bonds, int m, int mb, int LP, int* root_code,
                                              int* root_steps) {
  if (root_code)
    for (int r = 0; r < n && r < L; ++r) root_code[r] = -1, root_steps[r] = 0;
  if (!mol_graph_ok(bonds, n, nb, L, false) || !mol_graph_ok(p_bonds, m, mb, LP, true) || m > n) return kSubNone;
  uint64_t adj[kSubOrders * 64], compat[kSubMaxWidth];
  uint8_t back_start[kSubMaxWidth + 1], f[kSubMaxWidth], self_have[64], self_need[kSubMaxWidth];
  uint16_t back[kSubMaxWidth];
  for (int i = 0; i < kSubOrders * 64; ++i) adj[i] = 0;
  for (int e = 0; e < nb; ++e) {
    const int a = mol_a(bonds[e]), b = mol_b(bonds[e]), o = mol_order(bonds[e]);
    if (!mol_order_ok(o)) continue;                             // (no pattern entry asks for such an order)
    adj[(o - 1) * 64 + a] |= (uint64_t)1 << b;
    adj[(o - 1) * 64 + b] |= (uint64_t)1 << a;
  }
  for (int u = 0; u < n; ++u) {
    self_have[u] = 0;
    for (int o = 0; o < kSubOrders; ++o) self_have[u] |= (uint8_t)(((adj[o * 64 + u] >> u) & 1u) << o);
  }
  int k = 0;                                                    // the back-bonds grouped by their later atom
  for (int p = 0; p < m; ++p) {
    back_start[p] = (uint8_t)k;
    self_need[p] = 0;
    for (int e = 0; e < mb; ++e) {
      const int a = mol_a(p_bonds[e]), b = mol_b(p_bonds[e]), o = mol_order(p_bonds[e]);
      if ((a > b ? a : b) != p) continue;
      if (a == b) self_need[p] |= (uint8_t)(1u << (o - 1));     // an entry (p, p): part of what p accepts
      else back[k++] = (uint16_t)((a < b ? a : b) | o << 8);
    }
  }
  back_start[m] = (uint8_t)k;
  bool empty = false;
  for (int p = 0; p < m; ++p) {
    uint64_t c = 0;
    for (int u = 0; u < n; ++u)
      if (sub_accepts(p_atoms[p], atoms[u]) && (self_need[p] & ~self_have[u]) == 0) c |= (uint64_t)1 << u;
    compat[p] = c;
    empty = empty || c == 0;
  }
  if (empty) return kSubNone;
  if (m == 1) return kSubFound;
  const SubTables t{compat, adj, back_start, back, f, 1};
  bool found = false, capped = false;
  for (int r = 0; r < n; ++r) {
    if (!((compat[0] >> r) & 1u)) continue;
    int steps;
    SubNoSignal alone;
    const int code = sub_root_search(t, m, r, steps, alone);
    if (root_code) root_code[r] = code, root_steps[r] = steps;
    found = found || code == kSubFound;
    capped = capped || code == kSubCapped;
  }
  return found ? kSubFound : (capped ? kSubCapped : kSubNone);
}

}  // namespace mdt
