// One set of graph arrays for the Kekule, the aromatic and the bracket spelling of a molecule: the normal form of a graph row on
// gfx950, on the graph arrays of k_mol_graph, the hydrogens and the Kekule structure of k_mol_hydrogens and the ring sizes of
// k_mol_rings.  The definition -- the Kekule view, the pi electrons an atom gives, the two rings tried for an entry, Hueckel's count,
// the words written -- is written out at mdt_mol_normalize in include/mdt_hip.h; the per-atom rule, the Hueckel test, the output
// words and the serial form of the search are mdt_molnorm.h's, which a host program runs.
//
// k_mol_normalize: one wave per row, LANE = ATOM (and, for the per-entry outputs, lane = bond entry), four rows (waves) per
// workgroup, no barrier and NO LDS.  The bond list is wave-uniform (scalar loads); every lane takes the entries that touch it into
// its 64-bit adjacency word and its counts.  The search for one entry (a, b) is k_mol_rings': the visited set and the frontier are
// 64-bit scalar words, one level is  next = ballot((own & frontier) != 0) & ~visited,  and here every lane also keeps the level at
// which it was reached.  The walk back from b is one ballot per level -- the lanes of that level that are neighbours of the atom
// the walk stands on -- of which the lowest, in the second walk the highest, set bit is taken.  Hueckel's sum is
// popc(ring & ones) + 2 * popc(ring & twos); a ring that passes is OR-ed into the aromatic atom word, and lane e marks its own entry
// when both its ends are in that ring.  EVERY LOOP IS BOUNDED BY nb OR n: at most nb searches of at most n levels, two walks of
// fewer levels each; there is no step cap.  Early exits: a row that is no molecule or whose verdict is not 0; a row without an
// eligible ring bond, which only folds its hydrogens; an entry with an ineligible end, which is never searched.  No dynamically
// indexed register array: 0 bytes of scratch.  Vector stores only.
#include "mdt_kernels.h"
#include "mdt_device.h"
#include "mdt_molnorm.h"
#include "../../include/mdt_hip.h"

namespace mdt {

constexpr int kMolnRowsPerBlock = 4;                           // waves (rows) of a workgroup
static_assert(kMolnNormalized == MDT_MOLN_NORMALIZED && kMolnAromatic == MDT_MOLN_AROMATIC && kMolnChanged == MDT_MOLN_CHANGED,
              "mdt_hip.h and mdt_molnorm.h agree");

__global__ __launch_bounds__(64 * kMolnRowsPerBlock) void k_mol_normalize(
    const int32_t* __restrict__ natoms, const uint32_t* __restrict__ atoms, const int32_t* __restrict__ nbonds,
    const uint32_t* __restrict__ bonds, const uint8_t* __restrict__ hydrogens, const uint8_t* __restrict__ partner,
    const uint8_t* __restrict__ verdict, const uint8_t* __restrict__ bond_ring, int L, int R, uint32_t* __restrict__ out_atoms,
    uint32_t* __restrict__ out_bonds, uint8_t* __restrict__ flags) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t row = (int64_t)blockIdx.x * kMolnRowsPerBlock + wave;
  if (row >= R) return;                                         // (a whole wave leaves; nothing below crosses waves)
  const int n = natoms[row], nb = nbonds[row];
  const uint32_t* row_bonds = bonds + row * L;
  const uint8_t* row_partner = partner + row * L;
  const uint8_t* row_ring = bond_ring + row * L;
  uint32_t* out_a = out_atoms + row * L;                        // lane < L <= 64: the whole row, one store of the wave each
  uint32_t* out_b = out_bonds + row * L;
  if (!mol_graph_ok_wave(row_bonds, n, nb, L, lane)) {          // the rule of k_mol_key: such a row is no molecule
    if (lane < L) out_a[lane] = 0u, out_b[lane] = 0u;
    if (lane == 0) flags[row] = 0;
    return;
  }
  const bool here = lane < n, entry = lane < nb;                // (n, nb <= L from here on)
  const uint32_t d = here ? atoms[row * L + lane] : 0u;
  const uint32_t my_word = entry ? row_bonds[lane] : 0u;
  if (verdict[row] != 0) {                                      // no Kekule structure to read: the row as written
    if (lane < L) out_a[lane] = d, out_b[lane] = my_word;
    if (lane == 0) flags[row] = 0;
    return;
  }
  const int h = here ? (int)hydrogens[row * L + lane] : 0;
  // ---- per atom: its neighbours in the ring graph and what its entries' Kekule orders say (bounded by nb <= L) ----
  uint64_t adj = 0;
  int dbl = 0, sigma = h, other = 0;
  bool high = false, dbl_in_ring = false;
  for (int e = 0; e < nb; ++e) {
    const uint32_t w = row_bonds[e];                            // the same word in every lane
    const int a = mol_a(w), b = mol_b(w), o = mol_order(w);     // (a, b < n <= 64)
    const int k = o != 5 ? o : moln_kekule(a, b, o, row_partner[a], row_partner[b]);
    const bool at = a == lane || b == lane, proper = at && a != b;
    if (a != b) adj |= (a == lane ? (uint64_t)1 << b : 0) | (b == lane ? (uint64_t)1 << a : 0);
    high = high || (at && (k == 3 || k == 4));
    sigma += proper ? 1 : 0;
    if (proper && k == 2) {
      ++dbl;
      dbl_in_ring = row_ring[e] != 0;
      other = a == lane ? b : a;
    }
  }
  const uint32_t other_d = __shfl(d, other, 64);                // (taken by the whole wave; read only where dbl == 1)
  const int p = here ? moln_pi(d, dbl, high, sigma, dbl_in_ring, other_d) : kMolnIneligible;
  const uint64_t eligible = __ballot(p != kMolnIneligible), ones = __ballot(p == 1), twos = __ballot(p == 2);
  // ---- per entry (lane = bond entry from here on, as well): its Kekule order, and is it worth a search? ----
  const int ea = mol_a(my_word), eb = mol_b(my_word), eo = mol_order(my_word);
  int my_k = eo;
  if (entry && eo == 5) my_k = moln_kekule(ea, eb, eo, row_partner[ea], row_partner[eb]);
  const bool tried = entry && ea != eb && row_ring[lane] != 0 && ((eligible >> ea) & 1u) && ((eligible >> eb) & 1u);
  uint64_t aromatic = 0;
  bool marked = false;
  for (uint64_t rest = __ballot(tried); rest; rest &= rest - 1) {   // at most nb searches; none in a row without an eligible ring bond
    const uint32_t w = row_bonds[mol_lowest(rest)];
    const int a = mol_a(w), b = mol_b(w);
    const uint64_t bit_a = (uint64_t)1 << a, bit_b = (uint64_t)1 << b;
    const uint64_t own = adj & ~(lane == a ? bit_b : 0) & ~(lane == b ? bit_a : 0);
    uint64_t visited = bit_a, frontier = bit_a;                 // (mol_search by the wave; why it is written out: k_molring.hip)
    int my_level = 0, depth = 0;                                // (0: lane a, and every lane this search has not reached)
    bool found = false;
    for (;;) {                                                  // bounded by n: a level adds an atom to `visited` or ends the search
      const uint64_t next = __ballot((own & frontier) != 0) & ~visited;
      if (next == 0) break;
      ++depth;
      my_level = ((next >> lane) & 1u) ? depth : my_level;
      if (next & bit_b) { found = true; break; }
      visited |= next;
      frontier = next;
    }
    if (!found) continue;                                       // (bond_ring said otherwise: not the ring sizes of this graph)
    uint64_t first = 0;
    for (int pick = 0; pick < 2; ++pick) {
      uint64_t ring = bit_a | bit_b;
      int at = b;
      for (int level = depth - 1; level >= 1; --level) {        // one ballot per level
        const uint64_t from = __ballot(my_level == level && ((own >> at) & 1u));
        if (from == 0) break;                                   // (cannot be: an atom of level k + 1 has a neighbour of level k)
        at = pick ? mol_highest(from) : mol_lowest(from);
        ring |= (uint64_t)1 << at;
      }
      if (pick && ring == first) break;                         // one smallest cycle through the entry: judged already
      first = ring;
      if (!moln_hueckel(ring, eligible, ones, twos)) continue;
      aromatic |= ring;
      marked = marked || (entry && ((ring >> ea) & 1u) && ((ring >> eb) & 1u));
    }
  }
  // ---- the normal form ----
  const bool now = (aromatic >> lane) & 1u;
  const int order = marked ? 5 : my_k;
  if (lane < L) {
    out_a[lane] = here ? moln_atom_word(d, h, now) : 0u;
    out_b[lane] = entry ? moln_bond_word(ea, eb, order) : 0u;
  }
  const bool changed = __any((here && now != ((d & kMolAromatic) != 0)) || (entry && order != eo));
  if (lane == 0)
    flags[row] = (uint8_t)(kMolnNormalized | (aromatic ? kMolnAromatic : 0) | (changed ? kMolnChanged : 0));
}

}  // namespace mdt

// ------------------------------------------------------------------------------------------------
// C ABI entry point of this translation unit (declared in include/mdt_hip.h)
// ------------------------------------------------------------------------------------------------
extern "C" int mdt_mol_normalize(const int32_t* natoms, const uint32_t* atoms, const int32_t* nbonds, const uint32_t* bonds,
                                 const uint8_t* hydrogens, const uint8_t* partner, const uint8_t* verdict, const uint8_t* bond_ring,
                                 int32_t L, int32_t R, uint32_t* out_atoms, uint32_t* out_bonds, uint8_t* flags, void* stream) {
  if (R < 0) return mdt_bad("mdt_mol_normalize: need R >= 0");
  if (L < 1 || L > mdt::kMolMaxL) return mdt_bad("mdt_mol_normalize: need 1 <= L <= 64");
  if (R == 0) return 0;
  if (!natoms || !atoms || !nbonds || !bonds || !hydrogens || !partner || !verdict || !bond_ring || !out_atoms || !out_bonds || !flags)
    return mdt_bad("mdt_mol_normalize: null pointer");
  const unsigned blocks = (unsigned)(((int64_t)R + mdt::kMolnRowsPerBlock - 1) / mdt::kMolnRowsPerBlock);
  hipLaunchKernelGGL(mdt::k_mol_normalize, dim3(blocks), dim3(64 * mdt::kMolnRowsPerBlock), 0, (hipStream_t)stream, natoms, atoms,
                     nbonds, bonds, hydrogens, partner, verdict, bond_ring, L, R, out_atoms, out_bonds, flags);
  return mdt_finish("mdt_mol_normalize");
}
