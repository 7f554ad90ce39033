// Which ring framework is a molecule built on?  The Murcko-style scaffold of a graph row on gfx950, on the graph arrays of
// k_mol_graph or of k_mol_normalize: the 2-core of the ring graph (the atoms on a cycle or on a path between two cycles), with mode
// bit 0 plus the atoms double-bonded to it, as graph arrays of their own that k_mol_key takes unchanged.  The definition -- the core,
// the exocyclic atoms, the kept entries, the renumbering, the H field of a kept bracket atom, the words written -- is written out
// at mdt_mol_scaffold in include/mdt_hip.h; the per-word helpers and the serial form are mdt_molscaf.h's, which a host program runs.
//
// k_mol_scaffold: one wave per row, LANE = ATOM (and, for the per-entry outputs, lane = bond entry), four rows (waves) per
// workgroup, no barrier and NO LDS.  The bond list is wave-uniform (scalar loads); every lane takes the entries that touch it into
// its 64-bit adjacency word, and those of order 2 into a second one.  The core is ONE wave-uniform word, one ballot a round:
// alive &= ~ballot(alive_lane && popc(adj & alive) <= 1), until a round removes nobody.  The exocyclic atoms are one more ballot
// (not in the core, double-bonded into it); what a kept bracket atom gains is one more pass over the entries, made only where some
// atom was pruned and the mode keeps the words.  The new index of an atom is the popcount of the kept word below it; kept atoms
// and entries are scattered to their new slots, and the lanes from the kept count up to L write the zeros, so no word is written
// twice.  EVERY LOOP IS BOUNDED BY nb OR n: two passes over the nb entries, at most n rounds (each removes an atom or is the
// last); there is no step cap and no undecided answer.  No dynamically indexed register array: 0 bytes of scratch.  Vector stores
// only.
#include "mdt_kernels.h"
#include "mdt_device.h"
#include "mdt_molscaf.h"
#include "../../include/mdt_hip.h"

namespace mdt {

constexpr int kMolsRowsPerBlock = 4;                           // waves (rows) of a workgroup
static_assert(kMolsExocyclic == MDT_MOLS_EXOCYCLIC && kMolsGeneric == MDT_MOLS_GENERIC && kMolsMolecule == MDT_MOLS_MOLECULE &&
                  kMolsScaffold == MDT_MOLS_SCAFFOLD && kMolsWhole == MDT_MOLS_WHOLE,
              "mdt_hip.h and mdt_molscaf.h agree");

__global__ __launch_bounds__(64 * kMolsRowsPerBlock) void k_mol_scaffold(
    const int32_t* __restrict__ natoms, const uint32_t* __restrict__ atoms, const int32_t* __restrict__ nbonds,
    const uint32_t* __restrict__ bonds, int L, int R, int mode, int32_t* __restrict__ out_natoms, uint32_t* __restrict__ out_atoms,
    int32_t* __restrict__ out_nbonds, uint32_t* __restrict__ out_bonds, uint8_t* __restrict__ atom_map,
    uint8_t* __restrict__ flags) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t row = (int64_t)blockIdx.x * kMolsRowsPerBlock + wave;
  if (row >= R) return;                                         // (a whole wave leaves; nothing below crosses waves)
  const int n = natoms[row], nb = nbonds[row];
  const uint32_t* row_bonds = bonds + row * L;
  uint32_t* out_a = out_atoms + row * L;                        // lane < L <= 64: the whole row, one store of the wave each
  uint32_t* out_b = out_bonds + row * L;
  uint8_t* out_m = atom_map + row * L;
  if (!mol_graph_ok_wave(row_bonds, n, nb, L, lane)) {          // the rule of k_mol_key: such a row is no molecule
    if (lane < L) out_a[lane] = 0u, out_b[lane] = 0u, out_m[lane] = 0;
    if (lane == 0) out_natoms[row] = 0, out_nbonds[row] = 0, flags[row] = 0;
    return;
  }
  const bool here = lane < n, entry = lane < nb;                // (n, nb <= L from here on)
  const uint32_t d = here ? atoms[row * L + lane] : 0u;
  const uint32_t my_word = entry ? row_bonds[lane] : 0u;
  // ---- per atom: its neighbours in the ring graph, and those an entry of order 2 names (bounded by nb <= L) ----
  uint64_t adj = 0, dbl = 0;
  for (int e = 0; e < nb; ++e) {
    const uint32_t w = row_bonds[e];                            // the same word in every lane
    const int a = mol_a(w), b = mol_b(w);                       // (a, b < n <= 64)
    const uint64_t far = a == b ? 0 : (a == lane ? (uint64_t)1 << b : 0) | (b == lane ? (uint64_t)1 << a : 0);
    adj |= far;
    dbl |= mol_order(w) == 2 ? far : 0;
  }
  // ---- the core: in rounds, every atom with at most one neighbour still present leaves (bounded by n) ----
  uint64_t alive = __ballot(here);
  for (;;) {
    const uint64_t gone = __ballot(mol_in(alive, lane) && mol_popc(adj & alive) <= 1);
    if (gone == 0) break;
    alive &= ~gone;
  }
  // ---- the exocyclic atoms, the kept word, and what a kept bracket atom gains for the entries it loses ----
  uint64_t kept = alive;
  if (alive != 0 && (mode & kMolsExocyclic)) kept |= __ballot(here && !mol_in(alive, lane) && (dbl & alive) != 0);
  const int kept_atoms = mol_popc(kept);
  int gained = 0;
  if (kept_atoms != 0 && kept_atoms != n && !(mode & kMolsGeneric))
    for (int e = 0; e < nb; ++e) {
      const uint32_t w = row_bonds[e];
      const int a = mol_a(w), b = mol_b(w);
      const bool lost = a != b && ((a == lane && !mol_in(kept, b)) || (b == lane && !mol_in(kept, a)));
      gained += lost ? mols_weight(mol_order(w)) : 0;
    }
  // ---- the scaffold: kept atoms and entries at their new slots, zeros from the kept counts up to L ----
  const bool mine = mol_in(kept, lane);
  const int to = mol_index(kept, lane);                        // (< kept_atoms <= n <= L where `mine`)
  const int ea = mol_a(my_word), eb = mol_b(my_word);
  const bool stays = entry && ea != eb && mol_in(kept, ea) && mol_in(kept, eb);
  const uint64_t kept_entries = __ballot(stays);
  const int kept_bonds = mol_popc(kept_entries);
  if (mine) out_a[to] = mols_atom_word(d, gained, mode);
  if (stays) out_b[mol_index(kept_entries, lane)] = mols_bond_word(kept, ea, eb, mol_order(my_word), mode);
  if (lane < L) {
    if (lane >= kept_atoms) out_a[lane] = 0u;
    if (lane >= kept_bonds) out_b[lane] = 0u;
    out_m[lane] = mine ? (uint8_t)(1 + to) : (uint8_t)0;
  }
  if (lane == 0) {
    out_natoms[row] = kept_atoms;
    out_nbonds[row] = kept_bonds;
    flags[row] = (uint8_t)mols_flags(kept_atoms, n);
  }
}

}  // namespace mdt

// ------------------------------------------------------------------------------------------------
// C ABI entry point of this translation unit (declared in include/mdt_hip.h)
// ------------------------------------------------------------------------------------------------
extern "C" int mdt_mol_scaffold(const int32_t* natoms, const uint32_t* atoms, const int32_t* nbonds, const uint32_t* bonds, int32_t L,
                                int32_t R, int32_t mode, int32_t* out_natoms, uint32_t* out_atoms, int32_t* out_nbonds,
                                uint32_t* out_bonds, uint8_t* atom_map, uint8_t* flags, void* stream) {
  if (R < 0) return mdt_bad("mdt_mol_scaffold: need R >= 0");
  if (L < 1 || L > mdt::kMolMaxL) return mdt_bad("mdt_mol_scaffold: need 1 <= L <= 64");
  if (mode < 0 || mode > mdt::kMolsModes) return mdt_bad("mdt_mol_scaffold: need 0 <= mode <= 3 (MDT_MOLS_EXOCYCLIC | MDT_MOLS_GENERIC)");
  if (R == 0) return 0;
  if (!natoms || !atoms || !nbonds || !bonds || !out_natoms || !out_atoms || !out_nbonds || !out_bonds || !atom_map || !flags)
    return mdt_bad("mdt_mol_scaffold: null pointer");
  const unsigned blocks = (unsigned)(((int64_t)R + mdt::kMolsRowsPerBlock - 1) / mdt::kMolsRowsPerBlock);
  hipLaunchKernelGGL(mdt::k_mol_scaffold, dim3(blocks), dim3(64 * mdt::kMolsRowsPerBlock), 0, (hipStream_t)stream, natoms, atoms,
                     nbonds, bonds, L, R, mode, out_natoms, out_atoms, out_nbonds, out_bonds, atom_map, flags);
  return mdt_finish("mdt_mol_scaffold");
}
