// Ring perception and the descriptors of a graph row (mdt_hip.h, mdt_mol_rings): the descriptor slots and the rules that fill them,
// the integer masses, and the serial form of the row.  The symbol and formula-slot accessors are mdt_molh.h's; the bond word, "is
// this a graph row?", the ring graph, its components and the per-bond search -- breadth first over 64-bit adjacency words, bounded
// by the row's atoms -- are mdt_molrow.h's.  Like those headers everything here is __host__ __device__ and touches only the arrays
// it is handed.  The kernel (k_molring.hip: one wave per row, lane = atom, visited set and frontier as wave-uniform 64-bit words)
// uses the atom rules and the masses as they stand and runs one level of the search as a ballot where mol_search walks the words;
// a host program
// (tools/molring_host_check.cpp: arrays of exactly their size) runs molr_row, which is the definition written down in order.
#pragma once

#include <cstdint>
#include <hip/hip_runtime.h>

#include "mdt_molh.h"
#include "mdt_molrow.h"

namespace mdt {

constexpr int kMolrDesc = 16;
enum {
  kMolrHeavy = 0, kMolrHetero, kMolrDonors, kMolrAcceptors, kMolrRotatable, kMolrRings, kMolrRingAtoms, kMolrRingBonds,
  kMolrSmallestRing, kMolrLargestRing, kMolrAromatic, kMolrAromaticOutside, kMolrSp3Carbons, kMolrCarbons, kMolrComponents,
  kMolrWeight
};

// ---- what an atom is, by its place in the formula (molh_slot: H 0, C 2, N 3, O 4; a two-letter symbol or '*' is none of them) ----
__host__ __device__ __forceinline__ bool molr_heavy(uint32_t d) { return molh_slot(d) != kMolhSlotH; }
__host__ __device__ __forceinline__ bool molr_carbon(uint32_t d) { return molh_slot(d) == 2; }
__host__ __device__ __forceinline__ bool molr_n_or_o(uint32_t d) { return molh_slot(d) == 3 || molh_slot(d) == 4; }
__host__ __device__ __forceinline__ bool molr_aromatic(uint32_t d) { return (d & kMolAromatic) != 0; }

// The mass of a formula slot of mdt_mol_hydrogens (H B C N O F P S Cl Br I) in milli-dalton: the standard atomic weights of
// mol_weight(), each rounded to the nearest integer; "other" (and anything beyond) weighs 0.
__host__ __device__ __forceinline__ int molr_mass(int slot) {
  return slot == 0 ? 1008 : slot == 1 ? 10810 : slot == 2 ? 12011 : slot == 3 ? 14007 : slot == 4 ? 15999 : slot == 5 ? 18998
         : slot == 6 ? 30974 : slot == 7 ? 32060 : slot == 8 ? 35450 : slot == 9 ? 79904 : slot == 10 ? 126904 : 0;
}

// The search of the definition for one entry (a, b), a != b: 1 + the length of a shortest path from a to b that does not use the
// edge {a, b}, 0 if there is none.
__host__ __device__ inline int molr_search(const uint64_t* adj, int n, int a, int b) {
  const int level = mol_search(adj, n, a, b, nullptr);
  return level ? level + 1 : 0;
}

// The components of the ring graph: one flood each; at most n passes in all.
__host__ __device__ inline int molr_components(const uint64_t* adj, int n) {
  int components = 0;
  for (uint64_t seen = 0; seen != mol_all(n); seen |= mol_component(adj, n, seen)) ++components;
  return components;
}

// One row in the order the definition is written down.  Reads atoms[0:n], bonds[0:nb], hydrogens[0:n], lo / hi [0:16] when given;
// writes bond_ring[0:L], atom_ring[0:L], desc[0:16] and nothing beyond.  -> the flag: 1 when the row is a molecule and a descriptor
// lies outside [lo, hi] (0 without bounds).
__host__ __device__ inline int molr_row(const uint32_t* atoms, const uint32_t* bonds, const uint8_t* hydrogens, int n, int nb, int L,
                                        const int32_t* lo, const int32_t* hi, uint8_t* bond_ring, uint8_t* atom_ring, int32_t* desc) {
  for (int a = 0; a < L; ++a) bond_ring[a] = atom_ring[a] = 0;
  for (int k = 0; k < kMolrDesc; ++k) desc[k] = 0;
  if (!mol_graph_ok(bonds, n, nb, L, false)) return 0;         // (n == 0 included: no molecule)
  uint64_t adj[kMolMaxL], heavy = 0, triple = 0, not_single = 0;
  mol_ring_adj(bonds, n, nb, adj);
  for (int e = 0; e < nb; ++e) {
    const int o = mol_order(bonds[e]);
    const uint64_t ends = mol_bit(mol_a(bonds[e])) | mol_bit(mol_b(bonds[e]));
    if (o == 3 || o == 4) triple |= ends;
    if (o != 1) not_single |= ends;
  }
  int edges2 = 0, weight = 0, h_sum = 0;
  for (int a = 0; a < n; ++a) {
    const uint32_t d = atoms[a];
    const int h = hydrogens[a];
    edges2 += mol_popc(adj[a]);
    if (molr_heavy(d)) heavy |= (uint64_t)1 << a, ++desc[kMolrHeavy];
    if (molr_heavy(d) && !molr_carbon(d)) ++desc[kMolrHetero];
    if (molr_n_or_o(d)) ++desc[kMolrAcceptors];
    if (molr_n_or_o(d) && h >= 1) ++desc[kMolrDonors];
    if (molr_aromatic(d)) ++desc[kMolrAromatic];
    if (molr_carbon(d)) ++desc[kMolrCarbons];
    if (molr_carbon(d) && !molr_aromatic(d) && !((not_single >> a) & 1u)) ++desc[kMolrSp3Carbons];
    h_sum += h;
    weight += molr_mass(molh_slot(d));
  }
  const int components = molr_components(adj, n);
  desc[kMolrComponents] = components;
  desc[kMolrRings] = edges2 / 2 - n + components;
  desc[kMolrWeight] = weight + h_sum * molr_mass(kMolhSlotH);
  for (int e = 0; e < nb; ++e) {
    const int a = mol_a(bonds[e]), b = mol_b(bonds[e]);
    const int ring = a == b ? 0 : molr_search(adj, n, a, b);
    bond_ring[e] = (uint8_t)ring;
    if (ring) {
      if (atom_ring[a] == 0 || ring < atom_ring[a]) atom_ring[a] = (uint8_t)ring;
      if (atom_ring[b] == 0 || ring < atom_ring[b]) atom_ring[b] = (uint8_t)ring;
      ++desc[kMolrRingBonds];
      if (desc[kMolrSmallestRing] == 0 || ring < desc[kMolrSmallestRing]) desc[kMolrSmallestRing] = ring;
      if (ring > desc[kMolrLargestRing]) desc[kMolrLargestRing] = ring;
    }
  }
  for (int e = 0; e < nb; ++e) {
    const int a = mol_a(bonds[e]), b = mol_b(bonds[e]);
    if (mol_order(bonds[e]) == 1 && bond_ring[e] == 0 && a != b && mol_popc(adj[a] & heavy) >= 2 && mol_popc(adj[b] & heavy) >= 2 &&
        !((triple >> a) & 1u) && !((triple >> b) & 1u))
      ++desc[kMolrRotatable];
  }
  for (int a = 0; a < n; ++a) {
    if (atom_ring[a]) ++desc[kMolrRingAtoms];
    if (molr_aromatic(atoms[a]) && !atom_ring[a]) ++desc[kMolrAromaticOutside];
  }
  if (!lo) return 0;
  for (int k = 0; k < kMolrDesc; ++k)
    if (desc[k] < lo[k] || desc[k] > hi[k]) return 1;
  return 0;
}

}  // namespace mdt
