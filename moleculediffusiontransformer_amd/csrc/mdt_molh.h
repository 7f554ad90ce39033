// Implicit hydrogens and the Kekule check (mdt_hip.h, mdt_mol_hydrogens): the per-atom rule, the slot of an atom in the formula, the
// pick of the search and the search itself with its step count; the bond word, the check made before anything else (mol_graph_ok)
// and the sets are mdt_molrow.h's.  Like that header everything here is __host__ __device__ and touches only the arrays it is handed.  The
// kernel (k_molh.hip: one wave per row, lane = atom, the sets as wave-uniform 64-bit words) uses the rule, the slot and the pick
// key as they stand and runs the search's loop with ballots where molh_search walks arrays; a host program
// (tools/molh_host_check.cpp: arrays of exactly their size) runs molh_row, which is the definition written down in order.
#pragma once

#include <cstdint>
#include <hip/hip_runtime.h>

#include "mdt_molrow.h"

namespace mdt {

constexpr int kMolhMaxSteps = 4096, kMolhFormula = 13;
enum { kMolhOk = 0, kMolhAromaticOvervalent = 1, kMolhNoKekule = 2, kMolhUndecided = 3 };
enum { kMolhSlotH = 0, kMolhSlotOther = 11, kMolhSlotCharge = 12 };

__host__ __device__ __forceinline__ int molh_charge(uint32_t d) { return (int)((d >> 12) & 31u) - 9; }
__host__ __device__ __forceinline__ int molh_bracket_h(uint32_t d) { return (int)((d >> 17) & 15u); }
// what an entry of this order adds to the sums of its two atoms: the order, an aromatic entry (5) counted as 1
__host__ __device__ __forceinline__ int molh_order1(int order) { return order == 5 ? 1 : order; }

// The normal valences of a symbol as a bit set (bit v: v is one): B {3}, C {4}, N {3, 5}, O {2}, P {3, 5}, S {2, 4, 6}, and for an
// atom that is not aromatic F Cl Br I {1}.  Every other symbol, '*' included, has none.
__host__ __device__ __forceinline__ uint32_t molh_valences(uint32_t d) {
  const int first = (int)(d & 31u), second = (int)((d >> 5) & 31u);
  const bool aromatic = (d & kMolAromatic) != 0;
  if (second == 0) {
    if (first == 1) return 1u << 3;                             // B
    if (first == 2) return 1u << 4;                             // C
    if (first == 13 || first == 15) return 1u << 3 | 1u << 5;   // N, P
    if (first == 14) return 1u << 2;                            // O
    if (first == 18) return 1u << 2 | 1u << 4 | 1u << 6;        // S
    if (!aromatic && (first == 5 || first == 8)) return 1u << 1;   // F, I
    return 0u;
  }
  if (!aromatic && ((first == 2 && second == 12) || (first == 1 && second == 18))) return 1u << 1;   // Cl, Br
  return 0u;
}
// The lists of an aromatic bracket atom by g' = group - charge: 13 {3}, 14 {4}, 15 {3, 5}, 16 {2, 4, 6}; b 13, c 14, n p 15, o s 16.
__host__ __device__ __forceinline__ uint32_t molh_group_valences(uint32_t d) {
  const int first = (int)(d & 31u), second = (int)((d >> 5) & 31u);
  int g = 0;
  if (second == 0) g = first == 1 ? 13 : first == 2 ? 14 : (first == 13 || first == 15) ? 15 : (first == 14 || first == 18) ? 16 : 0;
  if (g == 0) return 0u;
  g -= molh_charge(d);
  return g == 13 ? 1u << 3 : g == 14 ? 1u << 4 : g == 15 ? (1u << 3 | 1u << 5) : g == 16 ? (1u << 2 | 1u << 4 | 1u << 6) : 0u;
}
// the smallest valence of the set that is >= sum, or -1 (sum >= 0; the sets end at bit 6)
__host__ __device__ __forceinline__ int molh_at_least(uint32_t set, int sum) {
  if (sum > 6) return -1;
  const uint32_t left = (set >> sum) << sum;
  return left ? mol_lowest((uint64_t)left) : -1;
}

// The per-atom rule: the hydrogens atom d carries when its entries sum to sum1, whether it still wants a double bond, and whether
// it is aromatic-overvalent.
__host__ __device__ __forceinline__ void molh_atom(uint32_t d, int sum1, int& h, bool& wants, bool& over) {
  const bool aromatic = (d & kMolAromatic) != 0;
  wants = over = false;
  if (d & kMolBracket) {                                        // taken at its word; never overvalent
    h = molh_bracket_h(d);
    if (aromatic) {
      const int v = molh_at_least(molh_group_valences(d), sum1 + h);
      wants = v >= 0 && v - (sum1 + h) >= 1;
    }
    return;
  }
  const int v = molh_at_least(molh_valences(d), sum1);
  if (!aromatic) {
    h = v < 0 ? 0 : v - sum1;
    return;
  }
  over = v < 0;
  wants = v >= 0 && v - sum1 >= 1;
  h = v < 0 ? 0 : v - sum1 - (int)wants;
}

// the atom's place in the formula: H B C N O F P S Cl Br I, 11 for any other symbol ('*' included)
__host__ __device__ __forceinline__ int molh_slot(uint32_t d) {
  const int first = (int)(d & 31u), second = (int)((d >> 5) & 31u);
  if (second == 0)
    return first == 7 ? 0 : first == 1 ? 1 : first == 2 ? 2 : first == 13 ? 3 : first == 14 ? 4 : first == 5 ? 5 : first == 15 ? 6
           : first == 18 ? 7 : first == 8 ? 10 : kMolhSlotOther;
  return (first == 2 && second == 12) ? 8 : (first == 1 && second == 18) ? 9 : kMolhSlotOther;
}

// The search of the definition on the words adj[a] (the atoms of W joined to a by an edge; 0 for an atom outside W, no bit a) and
// W, |W| even: -> kMolhOk with pair[a] = 1 + the partner of a for a in W, kMolhNoKekule or kMolhUndecided; steps: the tries made.
// su / sv: the stack, |W| / 2 <= 32 entries each.  Every pass of the loop makes a try or takes one back: at most 2 * max_steps + 2.
__host__ __device__ inline int molh_search(const uint64_t* adj, int n, uint64_t W, int max_steps, uint8_t* su, uint8_t* sv,
                                           uint8_t* pair, int& steps) {
  uint64_t M = W, allowed = ~(uint64_t)0;
  int depth = 0, made = 0, code;
  for (;;) {                                                    // bounded by max_steps
    if (M == 0) { code = kMolhOk; break; }
    int u = -1, fewest = 65;
    for (int a = 0; a < n; ++a) {                               // the unmatched atom with the fewest unmatched neighbours, lowest first
      if (!((M >> a) & 1u)) continue;
      const int c = mol_popc(adj[a] & M);
      if (c < fewest) fewest = c, u = a;
    }
    const uint64_t cand = adj[u] & M & allowed;
    if (cand == 0) {                                            // back: the last pair returns, its atom goes on above its partner
      if (depth == 0) { code = kMolhNoKekule; break; }
      --depth;
      M |= (uint64_t)1 << su[depth] | (uint64_t)1 << sv[depth];
      allowed = mol_above(sv[depth]);
      continue;
    }
    if (made == max_steps) { code = kMolhUndecided; break; }
    const int v = mol_lowest(cand);
    ++made;
    su[depth] = (uint8_t)u;
    sv[depth] = (uint8_t)v;
    ++depth;
    M &= ~((uint64_t)1 << u | (uint64_t)1 << v);
    allowed = ~(uint64_t)0;
  }
  if (code == kMolhOk)
    for (int k = 0; k < depth; ++k) pair[su[k]] = (uint8_t)(1 + sv[k]), pair[sv[k]] = (uint8_t)(1 + su[k]);
  steps = made;
  return code;
}

// One row in the order the definition is written down.  Reads atoms[0:n], bonds[0:nb]; writes hydrogens[0:L], partner[0:L],
// formula[0:13] and nothing beyond.  -> the verdict; atom: the lowest aromatic-overvalent atom or -1; steps: the tries made.
__host__ __device__ inline int molh_row(const uint32_t* atoms, const uint32_t* bonds, int n, int nb, int L, int max_steps,
                                        uint8_t* hydrogens, uint8_t* partner, int32_t* formula, int& atom, int& steps) {
  for (int a = 0; a < L; ++a) hydrogens[a] = partner[a] = 0;
  for (int k = 0; k < kMolhFormula; ++k) formula[k] = 0;
  atom = -1;
  steps = 0;
  if (!mol_graph_ok(bonds, n, nb, L, false)) return kMolhOk;   // (n == 0 included: no molecule)
  int sum1[kMolMaxL];
  uint64_t adj[kMolMaxL], W = 0;
  for (int a = 0; a < n; ++a) sum1[a] = 0, adj[a] = 0;
  for (int e = 0; e < nb; ++e) {
    const int a = mol_a(bonds[e]), b = mol_b(bonds[e]), o = mol_order(bonds[e]);
    sum1[a] += molh_order1(o);
    sum1[b] += molh_order1(o);
    if (o == 5 && a != b) adj[a] |= (uint64_t)1 << b, adj[b] |= (uint64_t)1 << a;
  }
  for (int a = 0; a < n; ++a) {
    int h;
    bool wants, over;
    molh_atom(atoms[a], sum1[a], h, wants, over);
    hydrogens[a] = (uint8_t)h;
    if (wants) W |= (uint64_t)1 << a;
    if (over && atom < 0) atom = a;
    formula[kMolhSlotH] += h;
    formula[molh_slot(atoms[a])] += 1;
    formula[kMolhSlotCharge] += molh_charge(atoms[a]);
  }
  if (atom >= 0) return kMolhAromaticOvervalent;
  if (mol_popc(W) & 1) return kMolhNoKekule;
  for (int a = 0; a < n; ++a) adj[a] = ((W >> a) & 1u) ? adj[a] & W : 0;
  uint8_t su[kMolMaxL / 2], sv[kMolMaxL / 2];
  return molh_search(adj, n, W, max_steps, su, sv, partner, steps);
}

}  // namespace mdt
