// The normal form of a graph row (mdt_hip.h, mdt_mol_normalize): the Kekule view of an entry, what an atom gives to a ring's pi
// system, the two rings tried for an entry -- the breadth-first search of mol_search with every atom keeping its level, walked back
// by the lowest and by the highest predecessor -- Hueckel's count, and the words of the normal form.  The symbol fields and the
// charge are mdt_molh.h's; the bond word, "is this a graph row?", the sets, the ring graph and the search are mdt_molrow.h's.  Like
// those headers everything here is __host__ __device__ and touches only the arrays it is handed.  The kernel (k_molnorm.hip: one wave per row,
// lane = atom and lane = entry, the sets as wave-uniform 64-bit words) uses the per-atom rule, the Hueckel test and the output words
// as they stand and runs one level of the search and of the walk back as a ballot where moln_two_rings walks arrays; a host program
// (tools/molnorm_host_check.cpp: arrays of exactly their size) runs moln_row, which is the definition written down in order.
#pragma once

#include <cstdint>
#include <hip/hip_runtime.h>

#include "mdt_molh.h"
#include "mdt_molrow.h"

namespace mdt {

enum { kMolnNormalized = 1, kMolnAromatic = 2, kMolnChanged = 4 };
constexpr int kMolnIneligible = -1;
constexpr uint32_t kMolnHField = 15u << 17;

// The Kekule view: the order an entry has once the aromatic entries are told apart by `partner` of mdt_mol_hydrogens (pa, pb: the
// partner words of its two ends).
__host__ __device__ __forceinline__ int moln_kekule(int a, int b, int o, int pa, int pb) {
  return o != 5 ? o : (a != b && pa == 1 + b && pb == 1 + a) ? 2 : 1;
}

// g' = group - charge of the symbols that can be in an aromatic ring (B 13, C 14, N P 15, O S 16, either case), 0 for every other
// symbol ('*' and every two-letter symbol included).
__host__ __device__ __forceinline__ int moln_group(uint32_t d) {
  const int first = (int)(d & 31u), second = (int)((d >> 5) & 31u);
  const int g = second != 0 ? 0 : first == 1 ? 13 : first == 2 ? 14 : (first == 13 || first == 15) ? 15 : (first == 14 || first == 18) ? 16 : 0;
  return g == 0 ? 0 : g - molh_charge(d);
}
__host__ __device__ __forceinline__ bool moln_n_o_s(uint32_t d) {
  const int first = (int)(d & 31u);
  return ((d >> 5) & 31u) == 0 && (first == 13 || first == 14 || first == 18);
}

// The pi electrons atom d gives to a ring, kMolnIneligible for an atom no aromatic ring can hold.  dbl: its entries (a != b) of
// Kekule order 2; high: some entry at it has Kekule order 3 or 4; sigma: its entries (a != b) plus its hydrogens; dbl_in_ring and
// other (the descriptor of the far end) describe the one double entry and are read only when dbl == 1.
__host__ __device__ __forceinline__ int moln_pi(uint32_t d, int dbl, bool high, int sigma, bool dbl_in_ring, uint32_t other) {
  const int g = moln_group(d);
  if (g == 0 || high || dbl >= 2) return kMolnIneligible;
  if (dbl == 1) {
    if (dbl_in_ring) return 1;
    return ((d & 31u) == 2 && molh_charge(d) == 0 && moln_n_o_s(other)) ? 0 : kMolnIneligible;   // a neutral C of C=N, C=O, C=S
  }
  if ((g == 16 && sigma == 2) || (g == 15 && sigma == 3)) return 2;
  if (g == 13 && sigma == 3) return 0;
  return kMolnIneligible;
}

// Hueckel on one ring: every atom eligible and the electrons 2 mod 4 (ones / twos: the atoms that give 1 / 2).
__host__ __device__ __forceinline__ bool moln_hueckel(uint64_t ring, uint64_t eligible, uint64_t ones, uint64_t twos) {
  return (ring & ~eligible) == 0 && ((mol_popc(ring & ones) + 2 * mol_popc(ring & twos)) & 3) == 2;
}

// the words of the normal form
__host__ __device__ __forceinline__ uint32_t moln_atom_word(uint32_t d, int h, bool aromatic) {
  return (d & ~(kMolAromatic | kMolnHField)) | kMolBracket | (aromatic ? kMolAromatic : 0u) | (uint32_t)(h > 15 ? 15 : h) << 17;
}
__host__ __device__ __forceinline__ uint32_t moln_bond_word(int a, int b, int order) {
  return (uint32_t)a | (uint32_t)b << 8 | (uint32_t)order << 16;
}

// The two rings tried for the entry (a, b), a != b, on the words adj[0:n] of the ring graph: mol_search from a to b, every atom
// keeping the level at which it was reached (at_level[k]: the atoms of level k; n words), then back from b taking at every level
// the lowest-numbered neighbour of that level, and again the highest.  -> false when b is not reached.  Every step of a walk goes
// down a level: bounded by n.
__host__ __device__ inline bool moln_two_rings(const uint64_t* adj, int n, int a, int b, uint64_t* at_level, uint64_t& lowest,
                                               uint64_t& highest) {
  const int depth = mol_search(adj, n, a, b, at_level);
  if (depth == 0) return false;
  for (int pick = 0; pick < 2; ++pick) {
    uint64_t ring = mol_bit(a) | mol_bit(b);
    int at = b;
    for (int level = depth - 1; level >= 1; --level) {          // (an atom of level k + 1 has a neighbour of level k)
      const uint64_t from = adj[at] & at_level[level];
      at = pick ? mol_highest(from) : mol_lowest(from);
      ring |= mol_bit(at);
    }
    (pick ? highest : lowest) = ring;
  }
  return true;
}

// One row in the order the definition is written down.  Reads atoms[0:n], bonds[0:nb], hydrogens[0:n], partner[0:n],
// bond_ring[0:nb]; writes out_atoms[0:L], out_bonds[0:L] and nothing beyond.  -> the flags.
__host__ __device__ inline int moln_row(const uint32_t* atoms, const uint32_t* bonds, const uint8_t* hydrogens, const uint8_t* partner,
                                        int verdict, const uint8_t* bond_ring, int n, int nb, int L, uint32_t* out_atoms,
                                        uint32_t* out_bonds) {
  for (int a = 0; a < L; ++a) out_atoms[a] = out_bonds[a] = 0;
  if (!mol_graph_ok(bonds, n, nb, L, false)) return 0;         // (n == 0 included: no molecule)
  if (verdict != 0) {                                           // no Kekule structure to read: the row as written
    for (int a = 0; a < n; ++a) out_atoms[a] = atoms[a];
    for (int e = 0; e < nb; ++e) out_bonds[e] = bonds[e];
    return 0;
  }
  uint64_t adj[kMolMaxL], at_level[kMolMaxL], eligible = 0, ones = 0, twos = 0, aromatic = 0, marked = 0;
  int kekule[kMolMaxL];
  mol_ring_adj(bonds, n, nb, adj);
  for (int e = 0; e < nb; ++e) {
    const int a = mol_a(bonds[e]), b = mol_b(bonds[e]);
    kekule[e] = moln_kekule(a, b, mol_order(bonds[e]), partner[a], partner[b]);
  }
  for (int x = 0; x < n; ++x) {
    int dbl = 0, sigma = hydrogens[x];
    bool high = false, dbl_in_ring = false;
    uint32_t other = 0;
    for (int e = 0; e < nb; ++e) {
      const int a = mol_a(bonds[e]), b = mol_b(bonds[e]);
      if (a != x && b != x) continue;
      high = high || kekule[e] == 3 || kekule[e] == 4;
      if (a == b) continue;
      ++sigma;
      if (kekule[e] == 2) ++dbl, dbl_in_ring = bond_ring[e] != 0, other = atoms[a == x ? b : a];
    }
    const int p = moln_pi(atoms[x], dbl, high, sigma, dbl_in_ring, other);
    if (p != kMolnIneligible) eligible |= (uint64_t)1 << x;
    if (p == 1) ones |= (uint64_t)1 << x;
    if (p == 2) twos |= (uint64_t)1 << x;
  }
  for (int e = 0; e < nb; ++e) {
    const int a = mol_a(bonds[e]), b = mol_b(bonds[e]);
    if (a == b || bond_ring[e] == 0 || !((eligible >> a) & 1u) || !((eligible >> b) & 1u)) continue;
    uint64_t ring[2];
    if (!moln_two_rings(adj, n, a, b, at_level, ring[0], ring[1])) continue;
    for (int pick = 0; pick < 2; ++pick) {
      if (!moln_hueckel(ring[pick], eligible, ones, twos)) continue;
      aromatic |= ring[pick];
      for (int f = 0; f < nb; ++f)
        if (((ring[pick] >> mol_a(bonds[f])) & 1u) && ((ring[pick] >> mol_b(bonds[f])) & 1u)) marked |= (uint64_t)1 << f;
    }
  }
  int flags = kMolnNormalized | (aromatic ? kMolnAromatic : 0);
  for (int x = 0; x < n; ++x) {
    const bool now = (aromatic >> x) & 1u;
    out_atoms[x] = moln_atom_word(atoms[x], hydrogens[x], now);
    if (now != ((atoms[x] & kMolAromatic) != 0)) flags |= kMolnChanged;
  }
  for (int e = 0; e < nb; ++e) {
    const int order = ((marked >> e) & 1u) ? 5 : kekule[e];
    out_bonds[e] = moln_bond_word(mol_a(bonds[e]), mol_b(bonds[e]), order);
    if (order != mol_order(bonds[e])) flags |= kMolnChanged;
  }
  return flags;
}

}  // namespace mdt
