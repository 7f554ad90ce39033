// The single-pass scanner of SMILES token rows that k_smiles.hip (the verdict) and k_molgraph.hip (the verdict and the molecular
// graph) share -- tokens -> graph row -- the graph key's per-root hash and the graph fingerprint.  The graph row itself (the
// descriptor, the bond word's accessors, "is this a graph row?") and the sets over it are mdt_molrow.h's.  The rules:
// include/mdt_hip.h, mdt_smiles_check and mdt_mol_graph / mdt_mol_key.  Everything here is __host__ __device__ and touches only the
// arrays it is handed, so the rules can be run, and their array bounds checked, in a host program without a device.  Included by
// .hip files only (mdt_api.cpp does not see it).
#pragma once

#include <cstdint>
#include <hip/hip_runtime.h>

#include "mdt_molrow.h"

namespace mdt {

// The class bytes (mdt_hip.h, mdt_smiles_check): 0 other | 1 + (c - 'A') | 27 + (c - 'a') | 53 + digit | then  - = # $ : / \ ( ) . [ ] % @ + *
constexpr int kClsUpper = 1, kClsLower = 27, kClsDigit = 53, kClsBond = 63, kClsOpen = 70, kClsClose = 71, kClsDot = 72,
              kClsLBracket = 73, kClsRBracket = 74, kClsPercent = 75, kClsAt = 76, kClsPlus = 77, kClsStar = 78;
constexpr int kClsMinus = kClsBond, kClsColon = kClsBond + 4;
enum { kPrevStart = 0, kPrevAtom, kPrevBond, kPrevDot, kPrevOpen, kPrevClose };
constexpr int kSmilesMaxL = 128, kSmilesRings = 100, kSmilesLanes = 64;
constexpr int kExempt = 127;                                   // capacity of an atom that is not judged (bracket, aromatic, '*')
constexpr int kNoPosition = 1 << 20;

__host__ __device__ __forceinline__ bool is_upper(int c) { return (unsigned)(c - kClsUpper) < 26u; }
__host__ __device__ __forceinline__ bool is_lower(int c) { return (unsigned)(c - kClsLower) < 26u; }
__host__ __device__ __forceinline__ bool is_digit(int c) { return (unsigned)(c - kClsDigit) < 10u; }
__host__ __device__ __forceinline__ bool is_bond(int c) { return (unsigned)(c - kClsBond) < 7u; }
// b c n o p s, as letters 0..25
__host__ __device__ __forceinline__ bool is_aromatic(int k) { return (unsigned)k < 26u && ((0x4E006u >> k) & 1u); }
// bond code 1..7 = - = # $ : / \ ; 0 = none, which bonds once
__host__ __device__ __forceinline__ int bond_order(int b) { return b >= 2 && b <= 4 ? b : 1; }
// The slot of an unbracketed uppercase atom in the max-valence table (B C N O P S F Cl Br I), -1: not an atom outside brackets.
__host__ __device__ __forceinline__ int organic_slot(int u) {
  switch (u) {
    case 'B' - 'A': return 0;
    case 'C' - 'A': return 1;
    case 'N' - 'A': return 2;
    case 'O' - 'A': return 3;
    case 'P' - 'A': return 4;
    case 'S' - 'A': return 5;
    case 'F' - 'A': return 6;
    case 'I' - 'A': return 9;
    default: return -1;
  }
}

// The per-lane bytes of LDS of k_smiles_check (see the top of k_smiles.hip) for rows of L positions: 4 * odd.
__host__ __device__ inline int smiles_lane_stride(int L) {
  const int bytes = L + L + (L + 1) / 2 + 2 * kSmilesRings;
  const int words = (bytes + 3) / 4;
  return 4 * (words | 1);
}

// The emitter of the scan that only judges: nothing is recorded, and what the scan computes for it alone is dead code.
struct SmilesNoEmit {
  static constexpr bool kEmits = false;
  __host__ __device__ __forceinline__ void atom(int, uint32_t) {}
  __host__ __device__ __forceinline__ void bond(int, int, int) {}
};

// The emitter that records the graph: atoms (descriptors, in order of appearance) and bonds (a | b << 8 | order << 16, in order
// of creation) into two arrays of L words, and per token position one byte -- the atom's index, bit 7: aromatic -- into `index`
// (L bytes).  An atom takes at least one token and a bond is made by an atom token or a closing ring token, so the counts stay
// <= L and <= L - 1.
struct MolGraphEmit {
  static constexpr bool kEmits = true;
  uint32_t* atoms;
  uint32_t* bonds;
  uint8_t* index;
  int natoms = 0, nbonds = 0;
  __host__ __device__ __forceinline__ void atom(int pos, uint32_t desc) {
    index[pos] = (uint8_t)(natoms | ((desc & kMolAromatic) ? 0x80 : 0));
    atoms[natoms++] = desc;
  }
  __host__ __device__ __forceinline__ void bond(int pos_a, int pos_b, int code) {
    const int a = index[pos_a], b = index[pos_b];
    const int order = mol_bond_order(code, (a & b & 0x80) != 0);
    bonds[nbonds++] = (uint32_t)(a & 63) | (uint32_t)(b & 63) << 8 | (uint32_t)order << 16;
  }
};

// The scan of one row (the rules: mdt_hip.h, mdt_smiles_check).  tok: its n <= L class bytes; cap (L), stack ((L + 1) / 2) and ring
// (2 * 100) are this row's work arrays, contents irrelevant before and after; limits: the ten maxima, one nibble each.
// -> the violation (>= 0: MALFORMED there) or -1, and `over`: the lowest overvalent atom or kNoPosition.  emit: told every atom
// (its token position and descriptor) as it appears, then every bond (the two atoms' positions and the bond code) as it is made;
// what it was told about a row that turns out malformed or overvalent is the caller's to discard.
template <class Emit>
__host__ __device__ inline int smiles_scan(const uint8_t* tok, int8_t* cap, uint8_t* stack, uint8_t* ring, int L, int n,
                                           uint64_t limits, const uint32_t* __restrict__ elements, int& over_out, Emit& emit) {
  const int depth_max = (L + 1) / 2;
  int prev = kPrevStart, bond_prev = kPrevStart, cur = 0, depth = 0, pending = 0;
  uint64_t open_lo = 0, open_hi = 0;
  int over = kNoPosition, viol = -1;

  // order `o` more on atom `a`: the capacity goes down; below zero the atom is overvalent, and stays so
  auto bond_to = [&](int a, int o) {
    int v = cap[a];
    if (v == kExempt) return;
    v -= o;
    if (v < -100) v = -100;
    cap[a] = (int8_t)v;
    if (v < 0 && a < over) over = a;
  };

  int j = 0;
  while (j < n && viol < 0) {
    const int c = tok[j];
    int atom_cap = -1;                                          // >= 0: tokens [j, next) are an atom of this capacity
    uint32_t desc = 0;                                          // ... and of this descriptor (used by an emitting scan only)
    int next = j + 1;
    if (is_upper(c)) {
      const int u = c - kClsUpper;
      int slot = organic_slot(u), second = 0;
      if (j + 1 < n) {
        const int d = tok[j + 1];
        if (u == 'C' - 'A' && d == kClsLower + ('l' - 'a')) { slot = 7; next = j + 2; second = 1 + ('l' - 'a'); }
        if (u == 'B' - 'A' && d == kClsLower + ('r' - 'a')) { slot = 8; next = j + 2; second = 1 + ('r' - 'a'); }
      }
      if (slot < 0) viol = j;
      else {
        atom_cap = (int)((limits >> (4 * slot)) & 15u);
        if constexpr (Emit::kEmits) desc = mol_descriptor(u, second, false, false, 0, 0, 0);
      }
    } else if (is_lower(c)) {
      if (is_aromatic(c - kClsLower)) {
        atom_cap = kExempt;
        if constexpr (Emit::kEmits) desc = mol_descriptor(c - kClsLower, 0, true, false, 0, 0, 0);
      } else {
        viol = j;
      }
    } else if (c == kClsStar) {
      atom_cap = kExempt;
      if constexpr (Emit::kEmits) desc = mol_descriptor(kMolStar, 0, false, false, 0, 0, 0);
    } else if (c == kClsLBracket) {
      int k = j + 1;
      int isotope = 0, first = 0, second = 0, charge = 0, hcount = 0;
      bool aromatic = false;
      while (k < n && is_digit(tok[k])) {                       // isotope
        if constexpr (Emit::kEmits) isotope = (isotope * 10 + (tok[k] - kClsDigit)) & 2047;
        ++k;
      }
      if (k >= n) viol = n;
      else {
        const int t = tok[k];
        if (is_upper(t)) {
          const uint32_t w = elements[t - kClsUpper];
          const int d = k + 1 < n ? tok[k + 1] : 0;
          first = t - kClsUpper;
          if (is_lower(d) && ((w >> (d - kClsLower)) & 1u)) { second = 1 + (d - kClsLower); k += 2; }
          else if ((w >> 26) & 1u) k += 1;
          else viol = k;
        } else if ((is_lower(t) && is_aromatic(t - kClsLower)) || t == kClsStar) {
          aromatic = t != kClsStar;
          first = aromatic ? t - kClsLower : kMolStar;
          k += 1;
        } else {
          viol = k;
        }
      }
      if (viol < 0) {
        if (k < n && tok[k] == kClsAt) {                        // chiral
          ++k;
          if (k < n && tok[k] == kClsAt) ++k;
        }
        if (k < n && tok[k] == kClsUpper + ('H' - 'A')) {       // hcount
          ++k;
          hcount = 1;
          if (k < n && is_digit(tok[k])) { hcount = tok[k] - kClsDigit; ++k; }
        }
        if (k < n && (tok[k] == kClsPlus || tok[k] == kClsMinus)) {   // charge
          const int sign = tok[k];
          ++k;
          charge = 1;
          if (k < n && (tok[k] == sign || is_digit(tok[k]))) { charge = tok[k] == sign ? 2 : tok[k] - kClsDigit; ++k; }
          if (sign == kClsMinus) charge = -charge;
        }
        if (k < n && tok[k] == kClsColon) {                     // class
          ++k;
          if (k >= n) viol = n;
          else if (!is_digit(tok[k])) viol = k;
          else
            while (k < n && is_digit(tok[k])) ++k;
        }
        if (viol < 0) {
          if (k >= n) viol = n;
          else if (tok[k] != kClsRBracket) viol = k;
          else {
            atom_cap = kExempt;
            next = k + 1;
            if constexpr (Emit::kEmits) desc = mol_descriptor(first, second, aromatic, true, charge, hcount, isotope);
          }
        }
      }
    } else if (is_bond(c)) {
      if (prev == kPrevAtom || prev == kPrevClose || prev == kPrevOpen) {
        bond_prev = prev;
        pending = c - kClsBond + 1;
        prev = kPrevBond;
      } else {
        viol = j;
      }
    } else if (is_digit(c) || c == kClsPercent) {
      const bool after_atom = prev == kPrevAtom || prev == kPrevClose;
      if (!(after_atom || (prev == kPrevBond && (bond_prev == kPrevAtom || bond_prev == kPrevClose)))) {
        viol = j;
      } else {
        int number = c - kClsDigit, last = j;
        if (c == kClsPercent) {
          if (j + 1 >= n) viol = n;
          else if (!is_digit(tok[j + 1])) viol = j + 1;
          else if (j + 2 >= n) viol = n;
          else if (!is_digit(tok[j + 2])) viol = j + 2;
          else {
            number = 10 * (tok[j + 1] - kClsDigit) + (tok[j + 2] - kClsDigit);
            last = j + 2;
          }
        }
        if (viol < 0) {                                         // 0 <= number <= 99
          const bool high = number >= 64;
          const uint64_t bit = (uint64_t)1 << (number & 63);
          if (!((high ? open_hi : open_lo) & bit)) {
            ring[2 * number] = (uint8_t)cur;
            ring[2 * number + 1] = (uint8_t)pending;
          } else {
            const int a = ring[2 * number], b = ring[2 * number + 1];
            if (a == cur || (b && pending && b != pending && !(b >= 6 && pending >= 6))) {
              viol = last;
            } else {
              const int o = bond_order(b ? b : pending);
              bond_to(a, o);
              bond_to(cur, o);
              emit.bond(a, cur, b ? b : pending);
            }
          }
          if (high) open_hi ^= bit; else open_lo ^= bit;
          pending = 0;
          prev = kPrevAtom;
          next = last + 1;
        }
      }
    } else if (c == kClsOpen) {
      if ((prev == kPrevAtom || prev == kPrevClose) && depth < depth_max) {   // (depth < depth_max always: two tokens per level)
        stack[depth++] = (uint8_t)cur;
        prev = kPrevOpen;
      } else {
        viol = j;
      }
    } else if (c == kClsClose) {
      if ((prev == kPrevAtom || prev == kPrevClose) && depth > 0) {
        cur = stack[--depth];
        prev = kPrevClose;
      } else {
        viol = j;
      }
    } else if (c == kClsDot) {
      if ((prev == kPrevAtom || prev == kPrevClose) && depth == 0) prev = kPrevDot;
      else viol = j;
    } else {
      viol = j;
    }
    if (atom_cap >= 0) {                                        // a new atom at position j
      cap[j] = (int8_t)atom_cap;
      emit.atom(j, desc);
      if (prev != kPrevStart && prev != kPrevDot) {
        const int o = bond_order(pending);
        bond_to(cur, o);
        bond_to(j, o);
        emit.bond(cur, j, pending);
      }
      pending = 0;
      cur = j;
      prev = kPrevAtom;
    }
    j = next;
  }
  if (viol < 0 && n > 0 && (!(prev == kPrevAtom || prev == kPrevClose) || depth > 0 || (open_lo | open_hi) != 0)) viol = n;

  over_out = over;
  return viol;
}

// ---- the graph key (mdt_hip.h, mdt_mol_key) ----
constexpr uint64_t kMolRoot = 0xA5A5A5A5A5A5A5A5ull, kMolBondK = 0x100000001B3ull;

// one splitmix64 step, as mdt_tokens_compact's
__host__ __device__ __forceinline__ uint64_t mol_mix(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// H_root of the graph (atoms[0:n], bonds[0:nb]): n rounds of refinement from the labelling that marks atom `root`.  lab and acc
// are this root's columns, element a at [a * stride] (n elements each; contents irrelevant before and after).  root >= n marks
// no atom; the caller discards that result.  Control flow and every bond depend on the graph alone, never on the root: on the
// device 64 roots walk in step, one per lane, with stride 64.
__host__ __device__ inline uint64_t mol_root_hash(const uint32_t* __restrict__ atoms, const uint32_t* __restrict__ bonds, int n,
                                                  int nb, int root, uint64_t* lab, uint64_t* acc, int stride) {
  for (int a = 0; a < n; ++a) {
    const uint64_t seed = mol_mix((uint64_t)atoms[a]);
    lab[a * stride] = a == root ? mol_mix(seed ^ kMolRoot) : seed;
    acc[a * stride] = 0;
  }
  for (int round = 0; round < n; ++round) {
    for (int e = 0; e < nb; ++e) {
      const uint32_t w = bonds[e];
      const int a = mol_a(w), b = mol_b(w);
      const uint64_t ok = (uint64_t)mol_order(w) * kMolBondK;
      const uint64_t la = lab[a * stride], lb = lab[b * stride];
      acc[a * stride] += mol_mix(lb + ok);
      acc[b * stride] += mol_mix(la + ok);
    }
    for (int a = 0; a < n; ++a) {
      lab[a * stride] = mol_mix(lab[a * stride] ^ mol_mix(acc[a * stride]));
      acc[a * stride] = 0;
    }
  }
  uint64_t h = 0;
  for (int a = 0; a < n; ++a) h += mol_mix(lab[a * stride]);
  return h;
}

// the key from the sum over the roots of mix(H_root); never 0 for a molecule
__host__ __device__ __forceinline__ uint64_t mol_key_final(uint64_t sum, int n, int nb) {
  const uint64_t key = mol_mix(sum + (uint64_t)n + ((uint64_t)nb << 32));
  return key ? key : 1;
}

// ---- the graph fingerprint and its Tanimoto similarity (mdt_hip.h, mdt_mol_fp / mdt_fp_nearest) ----
constexpr int kFpBits = 1024, kFpWords = kFpBits / 64, kFpDwords = kFpBits / 32, kFpMaxRadius = 3;
constexpr uint32_t kFpSimDen = 65536;

__host__ __device__ __forceinline__ uint64_t fp_seed(uint32_t atom, int deg) { return mol_mix((uint64_t)atom | (uint64_t)deg << 32); }
// what a bond of this order adds to the sum of the atom at its one end, given the label of the atom at its other end
__host__ __device__ __forceinline__ uint64_t fp_bond_term(uint64_t other, uint32_t order) {
  return mol_mix(other + (uint64_t)order * kMolBondK);
}
__host__ __device__ __forceinline__ uint64_t fp_next(uint64_t id, uint64_t acc) { return mol_mix(id ^ mol_mix(acc)); }
__host__ __device__ __forceinline__ int fp_bit(uint64_t id) { return (int)(id & (uint64_t)(kFpBits - 1)); }
// The fingerprint of one row, atom after atom: fp[0:16], returns the number of set bits.  This is the definition in the order it is
// written down; k_mol_fp computes the same with one atom per lane.  atoms[0:n], bonds[0:nb] are read, nothing beyond.
__host__ __device__ inline int fp_row(const uint32_t* atoms, const uint32_t* bonds, int n, int nb, int L, int radius, uint64_t* fp) {
  for (int w = 0; w < kFpWords; ++w) fp[w] = 0;
  if (!mol_graph_ok(bonds, n, nb, L, false)) return 0;
  uint64_t id[kMolMaxL], acc[kMolMaxL];
  int deg[kMolMaxL];
  for (int a = 0; a < n; ++a) deg[a] = 0;
  for (int e = 0; e < nb; ++e) {
    ++deg[mol_a(bonds[e])];
    ++deg[mol_b(bonds[e])];
  }
  for (int a = 0; a < n; ++a) id[a] = fp_seed(atoms[a], deg[a]);
  for (int r = 0;; ++r) {
    for (int a = 0; a < n; ++a) fp[fp_bit(id[a]) >> 6] |= 1ull << (fp_bit(id[a]) & 63);
    if (r == radius) break;
    for (int a = 0; a < n; ++a) acc[a] = 0;
    for (int e = 0; e < nb; ++e) {
      const uint32_t w = bonds[e];
      const int a = mol_a(w), b = mol_b(w);
      const uint64_t ta = fp_bond_term(id[b], mol_order(w)), tb = fp_bond_term(id[a], mol_order(w));
      acc[a] += ta;
      acc[b] += tb;
    }
    for (int a = 0; a < n; ++a) id[a] = fp_next(id[a], acc[a]);
  }
  int count = 0;
  for (int w = 0; w < kFpWords; ++w) count += mol_popc(fp[w]);
  return count;
}
// inter = |A & B|, uni = |A| + |B| - inter for two fingerprints of 16 words
__host__ __device__ inline void fp_counts(const uint64_t* a, const uint64_t* b, int& inter, int& uni) {
  int i = 0, ca = 0, cb = 0;
  for (int w = 0; w < kFpWords; ++w) {
    i += mol_popc(a[w] & b[w]);
    ca += mol_popc(a[w]);
    cb += mol_popc(b[w]);
  }
  inter = i;
  uni = ca + cb - i;
}
// "at least as similar as sim_num / 65536": exact, inside 32 bits (inter <= 1024, uni <= 2048, sim_num <= 65536)
__host__ __device__ __forceinline__ bool fp_at_least(int inter, int uni, uint32_t sim_num) {
  return uni > 0 && (uint32_t)inter * kFpSimDen >= sim_num * (uint32_t)uni;
}
// inter_a / uni_a > inter_b / uni_b, exact by cross-multiplication.  b is a running best that starts at (0, 1); a may be (0, 0) --
// two empty fingerprints, similarity 0 -- which is never greater.
__host__ __device__ __forceinline__ bool fp_greater(uint32_t inter_a, uint32_t uni_a, uint32_t inter_b, uint32_t uni_b) {
  return inter_a * uni_b > inter_b * uni_a;
}
// One word per (similarity, known index) whose unsigned maximum is "the largest similarity, the lowest index": the quotient
// floor(inter * 2^31 / uni) orders distinct fractions of denominators <= 2048 strictly (they differ by >= 2^-22) and maps equal
// fractions to equal values.
__host__ __device__ __forceinline__ uint64_t fp_pack(int inter, int uni, uint32_t index) {
  const uint64_t q = uni > 0 ? ((uint64_t)inter << 31) / (uint64_t)uni : 0;
  return q << 32 | (uint64_t)(0xFFFFFFFFu - index);
}

}  // namespace mdt
