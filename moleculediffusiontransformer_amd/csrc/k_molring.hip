// Which bonds and atoms lie in a ring, how small is it, and is the molecule inside the caller's descriptor bounds?  Ring perception
// and sixteen integer descriptors on gfx950, on the graph arrays of k_mol_graph and the hydrogens of k_mol_hydrogens.  The definition
// -- the ring graph, the per-bond shortest cycle, every descriptor slot, the integer masses -- is written out at mdt_mol_rings in
// include/mdt_hip.h; the atom rules, the masses and the serial form of the search are mdt_molring.h's, which a host program runs.
//
// k_mol_rings: one wave per row, LANE = ATOM (and, for the per-entry outputs, lane = bond entry), four rows (waves) per workgroup,
// no barrier and NO LDS: a row that is no molecule leaves after its counts and one ballot.  The bond list is wave-uniform (scalar
// loads); every lane takes the entries that touch it into its 64-bit adjacency word.  The search for one entry (a, b) is
// wave-uniform: the visited set and the frontier are 64-bit scalar words, one level is
//   next = ballot((adj_lane & frontier) != 0) & ~visited
// with lanes a and b masking each other out of their own word for that search, and it stops when b is reached or the frontier is
// empty.  The components come from the same flood, started from the lowest atom not yet seen.  EVERY LOOP IS BOUNDED BY nb, n OR
// BOTH -- at most nb searches of at most n levels (a level either adds an atom to `visited` or ends the search), at most n flood
// levels in all -- so no step cap is needed and none exists.  Early exits: a row with E == n - components has no cycle and runs no
// search; an entry at an atom with one neighbour is a bridge.  The result of the search for entry e is kept by lane e and folded
// into the minima of lanes a and b with selects; the descriptors are ballots, popcounts and one wave sum (the hydrogens and the
// degrees together).  No dynamically indexed register array: 0 bytes of scratch.  Vector stores only.
#include "mdt_kernels.h"
#include "mdt_device.h"
#include "mdt_molring.h"
#include "../../include/mdt_hip.h"

namespace mdt {

constexpr int kMolrRowsPerBlock = 4;                           // waves (rows) of a workgroup
static_assert(kMolrDesc == MDT_MOLR_DESC && kMolrHeavy == MDT_MOLR_HEAVY_ATOMS && kMolrHetero == MDT_MOLR_HETERO_ATOMS &&
                  kMolrDonors == MDT_MOLR_DONORS && kMolrAcceptors == MDT_MOLR_ACCEPTORS && kMolrRotatable == MDT_MOLR_ROTATABLE_BONDS &&
                  kMolrRings == MDT_MOLR_RINGS && kMolrRingAtoms == MDT_MOLR_RING_ATOMS && kMolrRingBonds == MDT_MOLR_RING_BONDS &&
                  kMolrSmallestRing == MDT_MOLR_SMALLEST_RING && kMolrLargestRing == MDT_MOLR_LARGEST_RING &&
                  kMolrAromatic == MDT_MOLR_AROMATIC_ATOMS && kMolrAromaticOutside == MDT_MOLR_AROMATIC_OUTSIDE_RING &&
                  kMolrSp3Carbons == MDT_MOLR_SP3_CARBONS && kMolrCarbons == MDT_MOLR_CARBONS &&
                  kMolrComponents == MDT_MOLR_COMPONENTS && kMolrWeight == MDT_MOLR_WEIGHT,
              "mdt_hip.h and mdt_molring.h agree");

__global__ __launch_bounds__(64 * kMolrRowsPerBlock) void k_mol_rings(
    const int32_t* __restrict__ natoms, const uint32_t* __restrict__ atoms, const int32_t* __restrict__ nbonds,
    const uint32_t* __restrict__ bonds, const uint8_t* __restrict__ hydrogens, int L, int R, const int32_t* __restrict__ lo,
    const int32_t* __restrict__ hi, uint8_t* __restrict__ bond_ring, uint8_t* __restrict__ atom_ring, int32_t* __restrict__ desc,
    uint8_t* __restrict__ flags) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t row = (int64_t)blockIdx.x * kMolrRowsPerBlock + wave;
  if (row >= R) return;                                         // (a whole wave leaves; nothing below crosses waves)
  const int n = natoms[row], nb = nbonds[row];
  const uint32_t* row_bonds = bonds + row * L;
  uint8_t* out_b = bond_ring + row * L;                         // lane < L <= 64: the whole row, one store of the wave each
  uint8_t* out_a = atom_ring + row * L;
  int32_t* out_d = desc + row * kMolrDesc;
  if (!mol_graph_ok_wave(row_bonds, n, nb, L, lane)) {          // the rule of k_mol_key: such a row is no molecule
    if (lane < L) out_b[lane] = 0, out_a[lane] = 0;
    if (lane < kMolrDesc) out_d[lane] = 0;
    if (flags && lane == 0) flags[row] = 0;
    return;
  }
  // ---- per atom: its neighbours in the ring graph, and what its entries' orders say (bounded by nb <= L) ----
  uint64_t adj = 0;
  bool triple = false, not_single = false;
  for (int e = 0; e < nb; ++e) {
    const uint32_t w = row_bonds[e];                            // the same word in every lane
    const int a = mol_a(w), b = mol_b(w), o = mol_order(w);     // (a, b < n <= 64)
    const bool at = a == lane || b == lane;
    if (a != b) adj |= (a == lane ? (uint64_t)1 << b : 0) | (b == lane ? (uint64_t)1 << a : 0);
    triple = triple || (at && (o == 3 || o == 4));
    not_single = not_single || (at && o != 1);
  }
  const bool here = lane < n;
  const uint32_t d = here ? atoms[row * L + lane] : 0u;
  const int h = here ? (int)hydrogens[row * L + lane] : 0;
  const int degree = mol_popc(adj);                            // (0 in a lane beyond n: no entry names it)
  const bool heavy = here && molr_heavy(d), carbon = here && molr_carbon(d), n_or_o = here && molr_n_or_o(d);
  const bool aromatic = here && molr_aromatic(d);
  const uint64_t heavy_set = __ballot(heavy);
  // ---- the components: floods from the lowest atom not yet seen (bounded by n: every level reaches an atom) ----
  const uint64_t all = mol_all(n);
  uint64_t seen = 0;
  int components = 0;
  while (seen != all) {                                         // (mol_component_wave's flood without its `members`: the row's
    uint64_t frontier = mol_bit(mol_lowest(all & ~seen));       //  atoms are only counted here, and through the helper the two
    ++components;                                               //  loops came out 4 scalar instructions a component longer)
    while (frontier) {
      seen |= frontier;
      frontier = __ballot((adj & frontier) != 0) & ~seen;
    }
  }
  // ---- one wave sum: the hydrogens and the degrees (h <= 255 and degree <= 63 for each of <= 64 atoms) ----
  int both = h | degree << 16;
  for (int off = 32; off >= 1; off >>= 1) both += __shfl_xor(both, off, 64);
  const int h_sum = both & 0xFFFF, edges = both >> 17;
  const int rings = edges - n + components;
  // ---- per entry: the smallest cycle through it (at most nb searches of at most n levels) ----
  const uint32_t my_word = lane < nb ? row_bonds[lane] : 0u;    // lane = bond entry from here on, as well
  const uint64_t leaves = __ballot(degree == 1);
  int my_bond_ring = 0, my_atom_ring = 0, smallest = 0, largest = 0;
  if (rings > 0) {                                              // (E == n - components: a forest, every entry is a bridge)
    for (int e = 0; e < nb; ++e) {
      const uint32_t w = row_bonds[e];
      const int a = mol_a(w), b = mol_b(w);
      if (a == b || (((leaves >> a) | (leaves >> b)) & 1u)) continue;   // no edge; the only edge of one of its ends: a bridge
      // mol_search by the wave, written out here and in k_mol_normalize: that one keeps every lane's level and asks "reached?" after
      // "empty?", this one keeps nothing and asks in the other order; one form for both needs a flag or changes both kernels' code
      const uint64_t own = adj & ~(lane == a ? (uint64_t)1 << b : 0) & ~(lane == b ? (uint64_t)1 << a : 0);
      uint64_t visited = (uint64_t)1 << a, frontier = visited;
      int ring = 0;
      for (int depth = 1;; ++depth) {                           // bounded by n: a level adds an atom to `visited` or ends the search
        const uint64_t next = __ballot((own & frontier) != 0) & ~visited;
        if ((next >> b) & 1u) { ring = depth + 1; break; }
        if (next == 0) break;
        visited |= next;
        frontier = next;
      }
      if (ring == 0) continue;
      my_bond_ring = lane == e ? ring : my_bond_ring;
      if ((lane == a || lane == b) && (my_atom_ring == 0 || ring < my_atom_ring)) my_atom_ring = ring;
      smallest = (smallest == 0 || ring < smallest) ? ring : smallest;
      largest = ring > largest ? ring : largest;
    }
  }
  if (lane < L) out_b[lane] = (uint8_t)my_bond_ring, out_a[lane] = (uint8_t)my_atom_ring;
  // ---- the descriptors: ballots and popcounts ----
  const uint64_t turns = __ballot(mol_popc(adj & heavy_set) >= 2 && !triple);   // atoms a rotatable bond may end at
  const int ea = mol_a(my_word), eb = mol_b(my_word);
  const bool rotatable = lane < nb && mol_order(my_word) == 1 && my_bond_ring == 0 && ea != eb && ((turns >> ea) & 1u) &&
                         ((turns >> eb) & 1u);
  int weight = h_sum * molr_mass(kMolhSlotH);
  const int slot = here ? molh_slot(d) : -1;
#pragma unroll
  for (int k = 0; k < kMolhSlotOther; ++k) weight += mol_popc(__ballot(slot == k)) * molr_mass(k);
  // (every ballot is taken by the whole wave, outside the selects: inside `lane == k ? ... : ...` only lane k would vote)
  const int n_heavy = mol_popc(heavy_set), n_hetero = mol_popc(__ballot(heavy && !carbon));
  const int n_donors = mol_popc(__ballot(n_or_o && h >= 1)), n_acceptors = mol_popc(__ballot(n_or_o));
  const int n_rotatable = mol_popc(__ballot(rotatable));
  const int n_ring_atoms = mol_popc(__ballot(my_atom_ring > 0)), n_ring_bonds = mol_popc(__ballot(my_bond_ring > 0));
  const int n_aromatic = mol_popc(__ballot(aromatic)), n_outside = mol_popc(__ballot(aromatic && my_atom_ring == 0));
  const int n_sp3 = mol_popc(__ballot(carbon && !aromatic && !not_single)), n_carbons = mol_popc(__ballot(carbon));
  int mine = 0;
  mine = lane == kMolrHeavy ? n_heavy : mine;
  mine = lane == kMolrHetero ? n_hetero : mine;
  mine = lane == kMolrDonors ? n_donors : mine;
  mine = lane == kMolrAcceptors ? n_acceptors : mine;
  mine = lane == kMolrRotatable ? n_rotatable : mine;
  mine = lane == kMolrRings ? rings : mine;
  mine = lane == kMolrRingAtoms ? n_ring_atoms : mine;
  mine = lane == kMolrRingBonds ? n_ring_bonds : mine;
  mine = lane == kMolrSmallestRing ? smallest : mine;
  mine = lane == kMolrLargestRing ? largest : mine;
  mine = lane == kMolrAromatic ? n_aromatic : mine;
  mine = lane == kMolrAromaticOutside ? n_outside : mine;
  mine = lane == kMolrSp3Carbons ? n_sp3 : mine;
  mine = lane == kMolrCarbons ? n_carbons : mine;
  mine = lane == kMolrComponents ? components : mine;
  mine = lane == kMolrWeight ? weight : mine;
  if (lane < kMolrDesc) out_d[lane] = mine;
  if (flags) {                                                  // (wave-uniform pointers: the whole wave takes the branch)
    bool outside = false;
    if (lo && lane < kMolrDesc) outside = mine < lo[lane] || mine > hi[lane];
    const bool any_outside = __any(outside);
    if (lane == 0) flags[row] = any_outside ? (uint8_t)MDT_SCREEN_SUBSTRUCTURE : (uint8_t)0;
  }
}

}  // namespace mdt

// ------------------------------------------------------------------------------------------------
// C ABI entry point of this translation unit (declared in include/mdt_hip.h)
// ------------------------------------------------------------------------------------------------
extern "C" int mdt_mol_rings(const int32_t* natoms, const uint32_t* atoms, const int32_t* nbonds, const uint32_t* bonds,
                             const uint8_t* hydrogens, int32_t L, int32_t R, const int32_t* lo, const int32_t* hi, uint8_t* bond_ring,
                             uint8_t* atom_ring, int32_t* desc, uint8_t* flags, void* stream) {
  if (R < 0) return mdt_bad("mdt_mol_rings: need R >= 0");
  if (L < 1 || L > mdt::kMolMaxL) return mdt_bad("mdt_mol_rings: need 1 <= L <= 64");
  if ((lo == nullptr) != (hi == nullptr)) return mdt_bad("mdt_mol_rings: lo and hi are given together or not at all");
  if (R == 0) return 0;
  if (!natoms || !atoms || !nbonds || !bonds || !hydrogens || !bond_ring || !atom_ring || !desc)
    return mdt_bad("mdt_mol_rings: null pointer");
  const unsigned blocks = (unsigned)(((int64_t)R + mdt::kMolrRowsPerBlock - 1) / mdt::kMolrRowsPerBlock);
  hipLaunchKernelGGL(mdt::k_mol_rings, dim3(blocks), dim3(64 * mdt::kMolrRowsPerBlock), 0, (hipStream_t)stream, natoms, atoms, nbonds,
                     bonds, hydrogens, L, R, lo, hi, bond_ring, atom_ring, desc, flags);
  return mdt_finish("mdt_mol_rings");
}
