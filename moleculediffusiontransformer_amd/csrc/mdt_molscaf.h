// The scaffold of a graph row (mdt_hip.h, mdt_mol_scaffold): the 2-core of the ring graph, the atoms double-bonded to it, what a
// kept bracket atom gains for the entries it loses, the renumbering and the words written.  The bracket atom's H count is
// mdt_molh.h's, the H field and the bond word are mdt_molnorm.h's, the descriptor, the bond accessors, "is this a graph row?" and
// the sets are mdt_molrow.h's.  Like those headers everything here is __host__ __device__ and touches only the arrays it is handed.  The
// kernel (k_molscaf.hip: one wave per row, lane = atom and lane = entry, the sets as wave-uniform 64-bit words) uses the per-word
// helpers as they stand and runs one round of the peeling as a ballot where mols_row walks arrays; a host program
// (tools/molscaf_host_check.cpp: arrays of exactly their size) runs mols_row, which is the definition written down in order.
#pragma once

#include <cstdint>
#include <hip/hip_runtime.h>

#include "mdt_molh.h"
#include "mdt_molnorm.h"
#include "mdt_molrow.h"

namespace mdt {

enum { kMolsExocyclic = 1, kMolsGeneric = 2, kMolsModes = 3 };              // the mode bits, and all of them
enum { kMolsMolecule = 1, kMolsScaffold = 2, kMolsWhole = 4 };              // the flag bits

// what a kept bracket atom gains in hydrogens for an entry of this order whose other end is pruned
__host__ __device__ __forceinline__ int mols_weight(int o) { return (o >= 1 && o <= 4) ? o : 1; }

// The word of a kept atom: with GENERIC the unbracketed C of mdt_mol_graph; otherwise as written, but for a bracket atom, whose H
// field takes the entries it lost (clamped at 15).
__host__ __device__ __forceinline__ uint32_t mols_atom_word(uint32_t d, int gained, int mode) {
  if (mode & kMolsGeneric) return mol_descriptor(2, 0, false, false, 0, 0, 0);
  if (!(d & kMolBracket)) return d;
  const int h = molh_bracket_h(d) + gained;
  return (d & ~kMolnHField) | (uint32_t)(h > 15 ? 15 : h) << 17;
}
// the word of a kept entry (a, b, o) under the renumbering of `kept`
__host__ __device__ __forceinline__ uint32_t mols_bond_word(uint64_t kept, int a, int b, int o, int mode) {
  return moln_bond_word(mol_index(kept, a), mol_index(kept, b), (mode & kMolsGeneric) ? 1 : o);
}
__host__ __device__ __forceinline__ int mols_flags(int kept_atoms, int n) {
  return kMolsMolecule | (kept_atoms > 0 ? kMolsScaffold : 0) | (kept_atoms == n ? kMolsWhole : 0);
}

// One row in the order the definition is written down.  Reads atoms[0:n], bonds[0:nb]; writes out_atoms[0:L], out_bonds[0:L],
// atom_map[0:L] and nothing beyond.  -> the flags; out_n / out_nb: the kept counts; rounds: the rounds that removed an atom.
__host__ __device__ inline int mols_row(const uint32_t* atoms, const uint32_t* bonds, int n, int nb, int L, int mode,
                                        uint32_t* out_atoms, uint32_t* out_bonds, uint8_t* atom_map, int& out_n, int& out_nb,
                                        int& rounds) {
  for (int a = 0; a < L; ++a) out_atoms[a] = out_bonds[a] = 0, atom_map[a] = 0;
  out_n = out_nb = rounds = 0;
  if (!mol_graph_ok(bonds, n, nb, L, false)) return 0;         // (n == 0 included: no molecule)
  uint64_t adj[kMolMaxL], dbl[kMolMaxL];                        // the ring graph, and its edges named by an entry of order 2
  for (int a = 0; a < n; ++a) adj[a] = dbl[a] = 0;
  for (int e = 0; e < nb; ++e) {
    const int a = mol_a(bonds[e]), b = mol_b(bonds[e]);
    if (a == b) continue;
    adj[a] |= (uint64_t)1 << b, adj[b] |= (uint64_t)1 << a;
    if (mol_order(bonds[e]) == 2) dbl[a] |= (uint64_t)1 << b, dbl[b] |= (uint64_t)1 << a;
  }
  uint64_t alive = mol_all(n);
  for (;;) {                                                    // bounded by n: a round removes an atom or is the last
    uint64_t gone = 0;
    for (int x = 0; x < n; ++x)
      if (mol_in(alive, x) && mol_popc(adj[x] & alive) <= 1) gone |= (uint64_t)1 << x;
    if (gone == 0) break;
    alive &= ~gone;
    ++rounds;
  }
  uint64_t kept = alive;
  if (alive != 0 && (mode & kMolsExocyclic))
    for (int x = 0; x < n; ++x)
      if (!mol_in(alive, x) && (dbl[x] & alive) != 0) kept |= (uint64_t)1 << x;
  for (int x = 0; x < n; ++x) {
    if (!mol_in(kept, x)) continue;
    int gained = 0;
    for (int e = 0; e < nb; ++e) {
      const int a = mol_a(bonds[e]), b = mol_b(bonds[e]);
      if (a != b && ((a == x && !mol_in(kept, b)) || (b == x && !mol_in(kept, a)))) gained += mols_weight(mol_order(bonds[e]));
    }
    const int to = mol_index(kept, x);
    out_atoms[to] = mols_atom_word(atoms[x], gained, mode);
    atom_map[x] = (uint8_t)(1 + to);
  }
  for (int e = 0; e < nb; ++e) {
    const int a = mol_a(bonds[e]), b = mol_b(bonds[e]);
    if (a != b && mol_in(kept, a) && mol_in(kept, b)) out_bonds[out_nb++] = mols_bond_word(kept, a, b, mol_order(bonds[e]), mode);
  }
  out_n = mol_popc(kept);
  return mols_flags(out_n, n);
}

}  // namespace mdt
