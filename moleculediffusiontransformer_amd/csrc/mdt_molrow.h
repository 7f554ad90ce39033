// The graph row and the sets over it: the atom descriptor, the bond word and "is this a graph row?" (mdt_hip.h, mdt_mol_graph), the
// 64-bit sets of atoms or entries that every molecule kernel works on, the ring graph of a row as adjacency words, its components
// and the search between the two ends of an entry.  Everything here but the _wave forms is __host__ __device__ and touches only
// the arrays it is handed, so the rules can be run, and their array bounds checked, in a host program without a device.  The
// _wave forms are the same steps by one wave that looks at one row, LANE = ATOM, the sets as wave-uniform words.  Everything is
// __forceinline__ or a plain loop: a kernel's code does not depend on whether a helper is defined here or in its file.
// The rule: what two molecule features use lives here, once; a new feature adds nothing here that it alone uses.
#pragma once

#include <cstdint>
#include <hip/hip_runtime.h>

namespace mdt {

// ---- the atom descriptor and the bond word of the molecular graph (mdt_hip.h, mdt_mol_graph) ----
constexpr int kMolMaxL = 64;                                   // at most 64 tokens: at most 64 atoms, at most 63 bonds
constexpr int kMolStar = 26;                                   // '*' in the first-letter field
constexpr uint32_t kMolAromatic = 1u << 10, kMolBracket = 1u << 11;
// first: letter 0..25 (either case) or kMolStar; second: 0 none, else 1 + (lowercase letter); charge in [-9, 9]; h in [0, 9];
// isotope already reduced modulo 2048
__host__ __device__ __forceinline__ uint32_t mol_descriptor(int first, int second, bool aromatic, bool bracket, int charge, int h,
                                                            int isotope) {
  return (uint32_t)first | (uint32_t)second << 5 | (aromatic ? kMolAromatic : 0u) | (bracket ? kMolBracket : 0u) |
         (uint32_t)(charge + 9) << 12 | (uint32_t)h << 17 | (uint32_t)isotope << 21;
}
// bond code (0 none, 1..7 = - = # $ : / \) -> the graph's order: - / \ 1, = 2, # 3, $ 4, ':' 5, none: 5 between two aromatic atoms, else 1
__host__ __device__ __forceinline__ int mol_bond_order(int code, bool both_aromatic) {
  if (code == 0) return both_aromatic ? 5 : 1;
  return code >= 2 && code <= 5 ? code : 1;
}
// the bond word a | b << 8 | order << 16, for every reader of the graph arrays
constexpr int kMolOrders = 5;                                  // the orders mol_bond_order writes: 1..5
__host__ __device__ __forceinline__ int mol_a(uint32_t w) { return (int)(w & 255u); }
__host__ __device__ __forceinline__ int mol_b(uint32_t w) { return (int)((w >> 8) & 255u); }
__host__ __device__ __forceinline__ int mol_order(uint32_t w) { return (int)(w >> 16); }
__host__ __device__ __forceinline__ bool mol_order_ok(int o) { return (unsigned)(o - 1) < (unsigned)kMolOrders; }
__host__ __device__ __forceinline__ bool mol_counts_ok(int n, int nb, int L) { return !(n < 1 || n > L || nb < 0 || nb > L); }
// Is (n, nb, bonds[0:nb]) the graph of a row of width L?  Counts inside [1, L] x [0, L], every bond end below n; with `orders`, also
// every order in 1..5 (asked of a substructure pattern: an entry of any other order, which mdt_mol_graph never writes, could not be
// satisfied).  A row that fails has no key, no fingerprint and matches nothing.  Reads bonds[0:nb] and nothing beyond.
__host__ __device__ inline bool mol_graph_ok(const uint32_t* bonds, int n, int nb, int L, bool orders) {
  if (!mol_counts_ok(n, nb, L)) return false;
  for (int e = 0; e < nb; ++e)
    if (mol_a(bonds[e]) >= n || mol_b(bonds[e]) >= n || (orders && !mol_order_ok(mol_order(bonds[e])))) return false;
  return true;
}
// mol_graph_ok (without `orders`) by one wave that looks at one row, lane e owning bond e (nb <= L <= 64): the wave-uniform
// verdict of k_mol_key and k_mol_fp.  Nothing is read when the counts already fail.  (k_sub_match spells the same check out with
// these accessors: it keeps the bond word, and through this helper its search came out 1-3 % slower on eight patterns.)
__device__ __forceinline__ bool mol_graph_ok_wave(const uint32_t* __restrict__ bonds, int n, int nb, int L, int lane) {
  const bool counts = mol_counts_ok(n, nb, L);
  const bool mine = counts && lane < nb;
  const uint32_t w = mine ? bonds[lane] : 0u;
  return counts && !__any(mine && (mol_a(w) >= n || mol_b(w) >= n));
}

// ---- sets of up to 64 atoms or entries as one word, bit i: member i ----
__host__ __device__ __forceinline__ int mol_popc(uint64_t w) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popcll((unsigned long long)w);
#else
  return __builtin_popcountll(w);
#endif
}
__host__ __device__ __forceinline__ int mol_lowest(uint64_t w) {           // the lowest member; w != 0
#if defined(__HIP_DEVICE_COMPILE__)
  return __ffsll((unsigned long long)w) - 1;
#else
  return __builtin_ctzll(w);
#endif
}
__host__ __device__ __forceinline__ int mol_highest(uint64_t w) {          // the highest member; w != 0
#if defined(__HIP_DEVICE_COMPILE__)
  return 63 - __clzll((long long)w);
#else
  return 63 - __builtin_clzll(w);
#endif
}
__host__ __device__ __forceinline__ uint64_t mol_bit(int i) { return (uint64_t)1 << i; }                    // {i}; i in 0..63
__host__ __device__ __forceinline__ uint64_t mol_below(int i) { return ((uint64_t)1 << i) - 1; }            // 0..i-1; i in 0..63
__host__ __device__ __forceinline__ uint64_t mol_above(int i) { return ~(((uint64_t)2 << i) - 1); }         // i+1..63; i in 0..63
// 0..n-1; n in 1..64 (0 gives the empty set).  The one place where a shift by 64 could be written.
__host__ __device__ __forceinline__ uint64_t mol_all(int n) { return n >= 64 ? ~(uint64_t)0 : mol_below(n); }
__host__ __device__ __forceinline__ bool mol_in(uint64_t set, int x) { return ((set >> x) & 1u) != 0; }    // x in 0..63
// the members of `set` below x (x in 0..63): the new index of member x once the set is numbered in ascending order
__host__ __device__ __forceinline__ int mol_index(uint64_t set, int x) { return mol_popc(set & mol_below(x)); }

// ---- the ring graph: atoms joined by an entry (a, b) with a != b, whatever its order, as one adjacency word per atom ----
// adj[0:n] from bonds[0:nb] of a row that mol_graph_ok accepts: bit c of adj[x]: {x, c} is an edge; symmetric, no bit x.
__host__ __device__ inline void mol_ring_adj(const uint32_t* bonds, int n, int nb, uint64_t* adj) {
  for (int a = 0; a < n; ++a) adj[a] = 0;
  for (int e = 0; e < nb; ++e) {
    const int a = mol_a(bonds[e]), b = mol_b(bonds[e]);
    if (a != b) adj[a] |= mol_bit(b), adj[b] |= mol_bit(a);
  }
}
// ... by one wave, lane = atom: -> the lane's word (0 in a lane beyond n: no entry names it).  The bond list is wave-uniform (scalar
// loads); every lane takes the entries that touch it.  A kernel that gathers more from the same pass keeps its own loop.
__device__ __forceinline__ uint64_t mol_ring_adj_wave(const uint32_t* __restrict__ row_bonds, int nb, int lane) {
  uint64_t adj = 0;
  for (int e = 0; e < nb; ++e) {
    const uint32_t w = row_bonds[e];                            // the same word in every lane
    const int a = mol_a(w), b = mol_b(w);
    if (a != b) adj |= (a == lane ? mol_bit(b) : 0) | (b == lane ? mol_bit(a) : 0);
  }
  return adj;
}

// The members of the component of the lowest atom not in `seen` (seen != mol_all(n): a union of whole components): a flood, one
// level a pass.  Every pass reaches an atom or is the last: the floods of a row take at most n passes in all.
__host__ __device__ inline uint64_t mol_component(const uint64_t* adj, int n, uint64_t seen) {
  uint64_t members = 0, frontier = mol_bit(mol_lowest(mol_all(n) & ~seen));
  while (frontier) {
    members |= frontier;
    uint64_t next = 0;
    for (int x = 0; x < n; ++x)
      if ((adj[x] & frontier) != 0) next |= mol_bit(x);
    frontier = next & ~members;
  }
  return members;
}
// ... by one wave, lane = atom: one ballot a level.  all: mol_all(n).
__device__ __forceinline__ uint64_t mol_component_wave(uint64_t adj_lane, uint64_t all, uint64_t seen) {
  uint64_t members = 0, frontier = mol_bit(mol_lowest(all & ~seen));
  while (frontier) {
    members |= frontier;
    frontier = __ballot((adj_lane & frontier) != 0) & ~members;
  }
  return members;
}

// The search for one entry (a, b), a != b, on the words adj[0:n] of the ring graph: breadth first from a, one level a pass, a and
// b not seeing each other -- the edge {a, b} is not used.  -> the level at which b is reached (so 1 + that level is the length of
// a smallest cycle through the entry), 0 when it is not.  at_level[k], when given: the atoms of level k, up to b's (at most n
// words: every level holds an atom of its own).  Every pass adds an atom to `visited` or ends the search: at most n - 1 passes.
__host__ __device__ inline int mol_search(const uint64_t* adj, int n, int a, int b, uint64_t* at_level) {
  uint64_t visited = mol_bit(a), frontier = visited;
  if (at_level) at_level[0] = visited;
  for (int depth = 1;; ++depth) {                               // bounded by n
    uint64_t next = 0;
    for (int x = 0; x < n; ++x) {
      uint64_t mine = adj[x];
      if (x == a) mine &= ~mol_bit(b);
      if (x == b) mine &= ~mol_bit(a);
      if (mine & frontier) next |= mol_bit(x);
    }
    next &= ~visited;
    if (next == 0) return 0;
    if (at_level) at_level[depth] = next;
    if (mol_in(next, b)) return depth;
    visited |= next;
    frontier = next;
  }
}

}  // namespace mdt
