// The canonical atom order of a graph row (mdt_hip.h, mdt_mol_canon): refinement with marks, the twin word, the target class of a
// node, the certificate of a leaf, and the serial form of the entry point -- an individualisation-refinement search over the
// refinement of mdt_mol_key, the smallest relabelled graph as the answer.  The mixing of the rooted hash is mdt_smiles_scan.h's; the
// bond accessors, "is this a graph row?", the sets, the ring graph and its components are mdt_molrow.h's.  Like those headers
// everything here is __host__ __device__ and touches only the arrays it is handed.  The kernel (k_molcanon.hip: one
// wave per row, lane = child of the node, then lane = atom and lane = entry for a leaf) uses molc_refine, molc_twin_key and
// molc_target as they stand and certifies a leaf with the whole wave where molc_certify walks arrays; a host program
// (tools/molcanon_host_check.cpp: arrays of exactly their size) runs molc_row.
#pragma once

#include <cstdint>
#include <hip/hip_runtime.h>

#include "mdt_molrow.h"
#include "mdt_smiles_scan.h"

namespace mdt {

enum { kMolcCanonical = 1, kMolcUndecided = 2 };               // the flags: one of them, or 0
constexpr int kMolcMaxNodes = 4096;
constexpr int kMolcNoMark = 255;                               // "no further mark" in a byte
constexpr int kMolcCertOne = 2 * kMolMaxL + 2;                 // one component: |C|, its words, the count, its entries
constexpr int kMolcCertAll = 4 * kMolMaxL;                     // all of a row: the sizes sum to <= 64, the counts to <= 64, 2 more each

// an entry of a certificate as one word that compares like (lo, hi, order): positions below 64, the order 16 bits
__host__ __device__ __forceinline__ uint32_t molc_entry(int pa, int pb, int order) {
  const int lo = pa < pb ? pa : pb, hi = pa < pb ? pb : pa;
  return (uint32_t)lo << 24 | (uint32_t)hi << 16 | (uint32_t)order;
}
// ... and the entry lo | hi << 8 | order << 16 of canon_bonds, `offset` added to both positions
__host__ __device__ __forceinline__ uint32_t molc_bond_word(uint32_t entry, int offset) {
  return ((entry >> 24) + (uint32_t)offset) | (((entry >> 16) & 255u) + (uint32_t)offset) << 8 | (entry & 0xFFFFu) << 16;
}

// The labels of the graph (atoms[0:n], bonds[0:nb]) after n rounds of refinement from the labelling that marks marks[0:k] in
// their order, then `last` as mark k (last >= n: no such mark).  lab and acc as in mol_root_hash, which this is with k = 0 and
// last = root.  Control flow and every bond depend on the graph and on k alone: on the device the children of a node walk in
// step, one per lane, each with its own `last`.
__host__ __device__ inline void molc_refine(const uint32_t* __restrict__ atoms, const uint32_t* __restrict__ bonds, int n, int nb,
                                            const uint8_t* marks, int k, int last, uint64_t* lab, uint64_t* acc, int stride) {
  for (int a = 0; a < n; ++a) {
    const uint64_t seed = mol_mix((uint64_t)atoms[a]);
    lab[a * stride] = a == last ? mol_mix(seed ^ (kMolRoot + (uint64_t)k)) : seed;
    acc[a * stride] = 0;
  }
  for (int j = 0; j < k; ++j) lab[marks[j] * stride] = mol_mix(mol_mix((uint64_t)atoms[marks[j]]) ^ (kMolRoot + (uint64_t)j));
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
}

// What twins share besides the atom word: the other end and the order of the ONE entry that names atom a; 0 when no entry or
// several name it (an entry (a, a) names a twice).
__host__ __device__ inline uint64_t molc_twin_key(const uint32_t* bonds, int nb, int a) {
  int named = 0;
  uint64_t key = 0;
  for (int e = 0; e < nb; ++e) {
    const uint32_t w = bonds[e];
    const uint64_t order = (uint64_t)mol_order(w) << 8 | (uint64_t)1 << 40;
    if (mol_a(w) == a) ++named, key = order | (uint64_t)mol_b(w);
    if (mol_b(w) == a) ++named, key = order | (uint64_t)mol_a(w);
  }
  return named == 1 ? key : 0;
}

// The target of a node from its labels (element a at lab[a * stride]): among the classes of equal label of the atoms of `open`
// (the component without the marks) that have at least 2 members and are not twin classes, the one with the smallest label -- 0:
// the node is a leaf.  twins[a]: the atoms that have a's twin key and a's word, a included; 0 when a has no twin key.
__host__ __device__ inline uint64_t molc_target(const uint64_t* lab, int stride, int n, uint64_t open, const uint64_t* twins) {
  uint64_t target = 0, least = 0;
  for (int a = 0; a < n; ++a) {
    const uint64_t la = lab[a * stride];
    if (!mol_in(open, a) || (target != 0 && la >= least)) continue;   // (la == least: the class already taken)
    uint64_t cls = 0;
    for (int b = 0; b < n; ++b)
      if (mol_in(open, b) && lab[b * stride] == la) cls |= (uint64_t)1 << b;
    if ((cls & (cls - 1)) != 0 && (cls & ~twins[a]) != 0) target = cls, least = la;
  }
  return target;
}

// The certificate of a leaf of the component `members` from its labels lab[0:n]: pos[a] for its atoms, cert[0:words] -> words.
__host__ __device__ inline int molc_certify(const uint64_t* lab, const uint32_t* atoms, const uint32_t* bonds, int n, int nb,
                                            uint64_t members, uint8_t* pos, uint32_t* cert) {
  const int size = mol_popc(members);
  cert[0] = (uint32_t)size;
  for (int a = 0; a < n; ++a) {
    if (!mol_in(members, a)) continue;
    int below = 0;
    for (int x = 0; x < n; ++x) below += (mol_in(members, x) && (lab[x] < lab[a] || (lab[x] == lab[a] && x < a))) ? 1 : 0;
    pos[a] = (uint8_t)below;
    cert[1 + below] = atoms[a];
  }
  int inside = 0;
  for (int e = 0; e < nb; ++e) {
    if (!mol_in(members, mol_a(bonds[e]))) continue;
    const uint32_t mine = molc_entry(pos[mol_a(bonds[e])], pos[mol_b(bonds[e])], mol_order(bonds[e]));
    int below = 0;
    for (int x = 0; x < nb; ++x) {
      if (!mol_in(members, mol_a(bonds[x]))) continue;
      const uint32_t other = molc_entry(pos[mol_a(bonds[x])], pos[mol_b(bonds[x])], mol_order(bonds[x]));
      below += (other < mine || (other == mine && x < e)) ? 1 : 0;
    }
    cert[2 + size + below] = mine;
    ++inside;
  }
  cert[1 + size] = (uint32_t)inside;
  return 2 + size + inside;
}

// is the leaf (cert, pos) better than the best one so far?  The smaller certificate; of two leaves with one certificate the one
// whose positions, read in ascending atom index, are the smaller sequence (so that the answer does not depend on the order in
// which the leaves are met).
__host__ __device__ inline bool molc_better(const uint32_t* cert, const uint32_t* best, int words, const uint8_t* pos,
                                            const uint8_t* best_pos, int n, uint64_t members) {
  for (int i = 0; i < words; ++i)
    if (cert[i] != best[i]) return cert[i] < best[i];
  for (int a = 0; a < n; ++a)
    if (mol_in(members, a) && pos[a] != best_pos[a]) return pos[a] < best_pos[a];
  return false;
}

// mdt_mol_canon of one row.  Reads atoms[0:n], bonds[0:nb]; writes priority[0:L], canon_atoms[0:L], canon_bonds[0:L] and nothing
// beyond.  -> the flags; nodes: the nodes of the search trees (kMolcMaxNodes + 1 for an undecided row).
__host__ __device__ inline int molc_row(const uint32_t* atoms, const uint32_t* bonds, int n, int nb, int L, uint64_t* priority,
                                        uint32_t* canon_atoms, uint32_t* canon_bonds, int32_t& nodes) {
  for (int a = 0; a < L; ++a) priority[a] = 0, canon_atoms[a] = 0, canon_bonds[a] = 0;
  nodes = 0;
  if (!mol_graph_ok(bonds, n, nb, L, false)) return 0;
  uint64_t lab[kMolMaxL], acc[kMolMaxL], adj[kMolMaxL], twin_key[kMolMaxL], twins[kMolMaxL];
  mol_ring_adj(bonds, n, nb, adj);
  for (int a = 0; a < n; ++a) twin_key[a] = molc_twin_key(bonds, nb, a);
  for (int a = 0; a < n; ++a) {
    twins[a] = 0;
    for (int b = 0; b < n; ++b)
      if (twin_key[a] != 0 && twin_key[b] == twin_key[a] && atoms[b] == atoms[a]) twins[a] |= (uint64_t)1 << b;
  }
  uint32_t certs[kMolcCertAll], cert[kMolcCertOne];             // the best certificate of every component, one after the other
  uint8_t best_pos[kMolMaxL], pos[kMolMaxL], marks[kMolMaxL];
  uint64_t pending[kMolMaxL];                                   // per level: the children of the node there that are still to visit
  int start[kMolMaxL], components = 0, used = 0, count = 0;
  uint64_t seen = 0, member_of[kMolMaxL];
  while (seen != mol_all(n)) {                                 // one component a turn
    const uint64_t members = mol_component(adj, n, seen);
    seen |= members;
    uint32_t* best = certs + used;
    bool have = false;
    int words = 0, level = 0;                                   // the node in hand has the marks marks[0:level]
    uint64_t marked = 0;
    for (;;) {                                                  // bounded by the node cap
      if (++count > kMolcMaxNodes) {                            // (nothing but zeros has been written)
        nodes = count;
        return kMolcUndecided;
      }
      molc_refine(atoms, bonds, n, nb, marks, level, kMolcNoMark, lab, acc, 1);
      pending[level] = molc_target(lab, 1, n, members & ~marked, twins);
      if (pending[level] == 0) {
        words = molc_certify(lab, atoms, bonds, n, nb, members, pos, cert);
        if (!have || molc_better(cert, best, words, pos, best_pos, n, members)) {
          for (int i = 0; i < words; ++i) best[i] = cert[i];
          for (int a = 0; a < n; ++a)
            if (mol_in(members, a)) best_pos[a] = pos[a];
          have = true;
        }
      }
      while (level >= 0 && pending[level] == 0) {               // back to the deepest level with a child to visit
        --level;
        if (level >= 0) marked &= ~((uint64_t)1 << marks[level]);
      }
      if (level < 0) break;
      const int child = mol_lowest(pending[level]);
      pending[level] &= pending[level] - 1;
      marks[level] = (uint8_t)child, marked |= (uint64_t)1 << child;
      ++level;
    }
    start[components] = used, member_of[components] = members;
    used += words;
    ++components;
  }
  nodes = count;
  // ---- the components in ascending (certificate, lowest atom): they were found in ascending lowest atom ----
  int offset = 0, entry_offset = 0;
  bool placed[kMolMaxL];
  for (int c = 0; c < components; ++c) placed[c] = false;
  for (int turn = 0; turn < components; ++turn) {
    int next = -1;
    for (int c = 0; c < components; ++c) {
      if (placed[c]) continue;
      if (next < 0) { next = c; continue; }
      const uint32_t *x = certs + start[c], *y = certs + start[next];
      int i = 0;                                                // (equal up to the shorter one's end only if equally long: the sizes lead)
      const int words = 2 + (int)x[0] + (int)x[1 + x[0]];
      while (i < words && x[i] == y[i]) ++i;
      if (i < words && x[i] < y[i]) next = c;
    }
    placed[next] = true;
    const uint32_t* x = certs + start[next];
    const int size = (int)x[0], inside = (int)x[1 + size];
    for (int a = 0; a < n; ++a)
      if (mol_in(member_of[next], a)) priority[a] = (uint64_t)(1 + offset + best_pos[a]), canon_atoms[offset + best_pos[a]] = atoms[a];
    for (int r = 0; r < inside; ++r) canon_bonds[entry_offset + r] = molc_bond_word(x[2 + size + r], offset);
    offset += size, entry_offset += inside;
  }
  return kMolcCanonical;
}

}  // namespace mdt
