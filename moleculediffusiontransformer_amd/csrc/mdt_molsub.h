// Graph substructure match (mdt_hip.h, mdt_sub_match): the atom rule and the depth-first search of one root with its step count;
// the bond word, the check made before any search (mol_graph_ok) and the sets are mdt_molrow.h's.  Like that header everything here is
// __host__ __device__ and touches only the arrays it is handed, so the kernel (k_molsub.hip: tables in LDS, one root per lane) and
// a host program (tools/molsub_host_check.cpp: tables in arrays of exactly their size) run the same search.
#pragma once

#include <cstdint>
#include <hip/hip_runtime.h>

#include "mdt_molrow.h"

namespace mdt {

constexpr int kSubMaxPatterns = 32, kSubMaxWidth = 32, kSubMaxSteps = 4096, kSubOrders = kMolOrders;
enum { kSubNone = 0, kSubFound = 1, kSubCapped = 2, kSubStopped = 3 };   // what one root's search ends with

// which bits of the descriptor pattern atom p compares: symbol and aromatic bit unless it is '*', charge, H count and isotope when it
// is bracketed; the bracket bit itself never
__host__ __device__ __forceinline__ uint32_t sub_atom_mask(uint32_t p) {
  return ((p & kMolBracket) ? 0xFFFFF000u : 0u) | ((p & 31u) == (uint32_t)kMolStar ? 0u : 0x7FFu);
}
__host__ __device__ __forceinline__ bool sub_accepts(uint32_t p, uint32_t t) { return ((p ^ t) & sub_atom_mask(p)) == 0; }

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
      cand = sub_candidates(t, p, used) & mol_above(last);
      continue;
    }
    if (made == kSubMaxSteps) { code = kSubCapped; break; }
    const int at = mol_lowest(cand);
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

// ---------------------------------------------------------------------------------------------------------------------
// Which atoms match, and how often (mdt_hip.h, mdt_sub_map): the same walk run to the END of a root's tree.  Additions only:
// everything above is mdt_sub_match's and stays as it is.
// ---------------------------------------------------------------------------------------------------------------------

// The enumeration of one root (2 <= m <= n, root in compat[0]): sub_root_search's walk, but at a success -- atom m - 1 assigned --
// sink.embedding(image) is told the set of target atoms of the full map (t.f holds the map itself at that moment) and the walk goes
// on at the same depth with the candidates above the one just taken.  -> the embeddings seen; capped: step kSubMaxSteps + 1 would
// have been made and the root was abandoned; steps: the assignments f(p) = t, p >= 1, made.  Up to the first success walk and step
// count are sub_root_search's, so "saw one" is its kSubFound and "capped and saw none" its kSubCapped.  No root stops for another.
// Every pass of the loop makes a step or takes one back, so it runs at most 2 * kSubMaxSteps + 2 times.
template <class Sink>
__host__ __device__ inline uint32_t sub_root_enumerate(const SubTables& t, int m, int root, int& steps, bool& capped, Sink& sink) {
  t.f[0] = (uint8_t)root;
  uint64_t used = (uint64_t)1 << root;                          // the images of the atoms below p
  int p = 1, made = 0;
  uint32_t seen = 0;
  bool cut = false;
  uint64_t cand = sub_candidates(t, 1, used);
  for (;;) {                                                    // bounded: at most kSubMaxSteps steps, and as many taken back
    if (cand == 0) {                                            // back: the next candidate of the atom before, above its last one
      --p;
      if (p == 0) break;
      const int last = t.f[p * t.f_stride];
      used &= ~((uint64_t)1 << last);
      cand = sub_candidates(t, p, used) & mol_above(last);
      continue;
    }
    if (made == kSubMaxSteps) { cut = true; break; }
    const int at = mol_lowest(cand);
    t.f[p * t.f_stride] = (uint8_t)at;
    ++made;
    if (p == m - 1) {                                           // a full map: report it, stay at this depth
      ++seen;
      sink.embedding(used | (uint64_t)1 << at);
      cand &= mol_above(at);
      continue;
    }
    used |= (uint64_t)1 << at;
    ++p;
    cand = sub_candidates(t, p, used);
  }
  steps = made;
  capped = cut;
  return seen;
}

// the sink that keeps the union of the images: one 64-bit OR an embedding
struct SubCoverSink {
  uint64_t cover;
  __host__ __device__ __forceinline__ void embedding(uint64_t image) { cover |= image; }
};

// Is the number of anchors of one (row, pattern) outside [lo, hi]?  c anchors are certain (roots that saw an embedding), u more are
// possible (roots abandoned before they saw one): outside unless lo <= c and c + u <= hi -- conservative both ways.  c + u <= 64,
// so hi >= 64 is no upper bound.
__host__ __device__ __forceinline__ bool sub_count_outside(uint64_t found, uint64_t capped, int lo, int hi) {
  const int c = mol_popc(found), u = mol_popc(capped & ~found);
  return !(lo <= c && c + u <= hi);
}

// One (row, pattern) pair of mdt_sub_map, root after root: found / capped (bit t: root t saw an embedding / was abandoned),
// embeddings (the maps seen over all roots), cover (every target atom in some map seen), map[0:LP] (1 + f(p) of the first map of
// the lowest found root, 0 elsewhere and beyond m); all zero for a pair decided "no match" before the search.  root_steps[0:n] /
// root_seen[0:n], when given, take every root's step count and embeddings (0 for a target atom that is no root).  The first map is
// handed out as k_sub_map does it: the lowest found root runs sub_root_search once more.  Reads atoms[0:n], bonds[0:nb],
// p_atoms[0:m], p_bonds[0:mb], writes map[0:LP], and nothing beyond.
__host__ __device__ inline void sub_map_pair(const uint32_t* atoms, const uint32_t* bonds, int n, int nb, int L,
                                             const uint32_t* p_atoms, const uint32_t* p_bonds, int m, int mb, int LP, uint64_t* found,
                                             uint64_t* capped, uint32_t* embeddings, uint64_t* cover, uint8_t* map, int* root_steps,
                                             uint32_t* root_seen) {
  *found = *capped = *cover = 0;
  *embeddings = 0;
  for (int p = 0; p < LP; ++p) map[p] = 0;                      // bounded by LP
  if (root_steps)
    for (int r = 0; r < n && r < L; ++r) root_steps[r] = 0, root_seen[r] = 0;
  if (!mol_graph_ok(bonds, n, nb, L, false) || !mol_graph_ok(p_bonds, m, mb, LP, true) || m > n) return;
  uint64_t adj[kSubOrders * 64], compat[kSubMaxWidth];
  uint8_t back_start[kSubMaxWidth + 1], f[kSubMaxWidth], self_have[64], self_need[kSubMaxWidth];
  uint16_t back[kSubMaxWidth];
  for (int i = 0; i < kSubOrders * 64; ++i) adj[i] = 0;
  for (int e = 0; e < nb; ++e) {                                // bounded by nb <= L
    const int a = mol_a(bonds[e]), b = mol_b(bonds[e]), o = mol_order(bonds[e]);
    if (!mol_order_ok(o)) continue;
    adj[(o - 1) * 64 + a] |= (uint64_t)1 << b;
    adj[(o - 1) * 64 + b] |= (uint64_t)1 << a;
  }
  for (int u = 0; u < n; ++u) {                                 // bounded by n <= L
    self_have[u] = 0;
    for (int o = 0; o < kSubOrders; ++o) self_have[u] |= (uint8_t)(((adj[o * 64 + u] >> u) & 1u) << o);
  }
  int k = 0;
  for (int p = 0; p < m; ++p) {                                 // bounded by m <= LP, inside by mb <= LP
    back_start[p] = (uint8_t)k;
    self_need[p] = 0;
    for (int e = 0; e < mb; ++e) {
      const int a = mol_a(p_bonds[e]), b = mol_b(p_bonds[e]), o = mol_order(p_bonds[e]);
      if ((a > b ? a : b) != p) continue;
      if (a == b) self_need[p] |= (uint8_t)(1u << (o - 1));
      else back[k++] = (uint16_t)((a < b ? a : b) | o << 8);
    }
  }
  back_start[m] = (uint8_t)k;
  bool empty = false;
  for (int p = 0; p < m; ++p) {                                 // bounded by m <= LP, inside by n <= L
    uint64_t c = 0;
    for (int u = 0; u < n; ++u)
      if (sub_accepts(p_atoms[p], atoms[u]) && (self_need[p] & ~self_have[u]) == 0) c |= (uint64_t)1 << u;
    compat[p] = c;
    empty = empty || c == 0;
  }
  if (empty) return;
  if (m == 1) {                                                 // every accepted atom is an anchor, a map and its own image
    *found = *cover = compat[0];
    *embeddings = (uint32_t)mol_popc(compat[0]);
    map[0] = (uint8_t)(1 + mol_lowest(compat[0]));
    return;
  }
  const SubTables t{compat, adj, back_start, back, f, 1};
  for (int r = 0; r < n; ++r) {                                 // bounded by n <= L; no root stops for another
    if (!((compat[0] >> r) & 1u)) continue;
    int steps;
    bool cut;
    SubCoverSink sink{0};
    const uint32_t seen = sub_root_enumerate(t, m, r, steps, cut, sink);
    if (root_steps) root_steps[r] = steps, root_seen[r] = seen;
    if (seen) *found |= (uint64_t)1 << r;
    if (cut) *capped |= (uint64_t)1 << r;
    *embeddings += seen;
    *cover |= sink.cover;
  }
  if (*found) {
    int steps;
    SubNoSignal alone;
    sub_root_search(t, m, mol_lowest(*found), steps, alone);    // (it succeeds: the enumeration of that root saw a map)
    for (int p = 0; p < m; ++p) map[p] = (uint8_t)(1 + f[p]);   // bounded by m <= LP
  }
}

}  // namespace mdt
