// How many hydrogens does each atom carry, and can the aromatic atoms' double bonds be placed?  Implicit hydrogens, a Kekule check
// and the molecular formula on gfx950, on the graph arrays of k_mol_graph.  The definition -- the per-atom rule, the order of the
// matching search and its step cap, which is what makes "undecided" a defined answer -- is written out at mdt_mol_hydrogens in
// include/mdt_hip.h; the rule, the formula slot and the serial form of the search are mdt_molh.h's, which a host program runs as well.
//
// k_mol_hydrogens: one wave per row, LANE = ATOM, four rows (waves) per workgroup, no barrier and NO LDS: a row that is no molecule
// leaves after its counts and one ballot.  The bond list is wave-uniform (scalar loads); every lane takes the entries that touch
// it: its sum and its adjacency word (64 bits: its order-5 neighbours).  The sets W (wanting) and M (unmatched) are wave-uniform
// 64-bit words built by ballots.  The search's control flow is wave-uniform: the pick of u is one popcount per lane and at most
// n ballots (count 0, 1, 2, ... -- an aromatic atom has at most three ring neighbours, so two or three in practice), its
// adjacency word is one readlane pair, the candidate is a find-first-set on scalars.  The stack is not stored: a matched lane
// keeps the depth at which it was matched in a register, so "restore the last pair" is one ballot; which of the two was u comes
// out of the pick on the restored set, which is the pick that chose it.  The formula is twelve ballots with popcounts and one wave
// sum that carries H and the charge together.  No dynamically indexed register array: 0 bytes of scratch.
#include "mdt_kernels.h"
#include "mdt_device.h"
#include "mdt_molh.h"
#include "../../include/mdt_hip.h"

namespace mdt {

constexpr int kMolhRowsPerBlock = 4;                           // waves (rows) of a workgroup
static_assert(kMolhMaxSteps == MDT_MOLH_MAX_STEPS && kMolhFormula == MDT_MOLH_FORMULA, "mdt_hip.h and mdt_molh.h agree");
static_assert(kMolhOk == MDT_MOLH_OK && kMolhAromaticOvervalent == MDT_MOLH_AROMATIC_OVERVALENT &&
                  kMolhNoKekule == MDT_MOLH_NO_KEKULE && kMolhUndecided == MDT_MOLH_UNDECIDED,
              "mdt_hip.h and mdt_molh.h agree");

__global__ __launch_bounds__(64 * kMolhRowsPerBlock) void k_mol_hydrogens(
    const int32_t* __restrict__ natoms, const uint32_t* __restrict__ atoms, const int32_t* __restrict__ nbonds,
    const uint32_t* __restrict__ bonds, int L, int R, int max_steps, uint8_t* __restrict__ hydrogens, uint8_t* __restrict__ partner,
    uint8_t* __restrict__ verdict, int32_t* __restrict__ atom, int32_t* __restrict__ formula) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t row = (int64_t)blockIdx.x * kMolhRowsPerBlock + wave;
  if (row >= R) return;                                         // (a whole wave leaves; nothing below crosses waves)
  const int n = natoms[row], nb = nbonds[row];
  const uint32_t* row_bonds = bonds + row * L;
  uint8_t* out_h = hydrogens + row * L;                         // lane < L <= 64: the whole row, one store of the wave each
  uint8_t* out_p = partner + row * L;
  int32_t* out_f = formula + row * kMolhFormula;
  if (!mol_graph_ok_wave(row_bonds, n, nb, L, lane)) {          // the rule of k_mol_key: such a row is no molecule
    if (lane < L) out_h[lane] = 0, out_p[lane] = 0;
    if (lane < kMolhFormula) out_f[lane] = 0;
    if (lane == 0) verdict[row] = (uint8_t)kMolhOk, atom[row] = -1;
    return;
  }
  // ---- per atom: the sum of its entries and its order-5 neighbours (bounded by nb <= L) ----
  int sum1 = 0;
  uint64_t adj = 0;
  for (int e = 0; e < nb; ++e) {
    const uint32_t w = row_bonds[e];                            // the same word in every lane
    const int a = mol_a(w), b = mol_b(w), o = mol_order(w);     // (a, b < n <= 64)
    const int o1 = molh_order1(o);
    sum1 += (a == lane ? o1 : 0) + (b == lane ? o1 : 0);        // (an entry (a, a) counts twice at a)
    if (o == 5 && a != b) adj |= (a == lane ? (uint64_t)1 << b : 0) | (b == lane ? (uint64_t)1 << a : 0);
  }
  const bool here = lane < n;
  const uint32_t desc = here ? atoms[row * L + lane] : 0u;
  int h;
  bool wants, over;
  molh_atom(desc, sum1, h, wants, over);
  h = here ? h : 0;
  const uint64_t W = __ballot(here && wants), overvalent = __ballot(here && over);
  adj = ((W >> lane) & 1u) ? adj & W : 0;                       // an edge joins two distinct atoms of W
  // ---- the formula: eleven symbols and "other" by ballots, H and the charge by one wave sum ----
  const int slot = here ? molh_slot(desc) : -1;
  int mine = 0;
#pragma unroll
  for (int k = 0; k < kMolhSlotCharge; ++k) {
    const int c = mol_popc(__ballot(slot == k));
    mine = lane == k ? c : mine;
  }
  int both = here ? (h | (molh_charge(desc) + 9) << 16) : 0;    // (h <= 15 and charge + 9 <= 31 for each of <= 64 atoms)
  for (int off = 32; off >= 1; off >>= 1) both += __shfl_xor(both, off, 64);
  mine = lane == kMolhSlotH ? mine + (both & 0xFFFF) : (lane == kMolhSlotCharge ? (both >> 16) - 9 * n : mine);
  if (lane < kMolhFormula) out_f[lane] = mine;
  // ---- the verdict ----
  int code, first_over = -1, my_depth = -1, my_partner = 0;
  if (overvalent) {
    code = kMolhAromaticOvervalent;
    first_over = mol_lowest(overvalent);
  } else if (mol_popc(W) & 1) {
    code = kMolhNoKekule;
  } else {
    uint64_t M = W, back = 0;                                   // back: the pair a step back has just restored, else 0
    int depth = 0, made = 0;
    for (;;) {                                                  // bounded: at most max_steps tries, and as many taken back
      if (M == 0) { code = kMolhOk; break; }
      const bool in = (M >> lane) & 1u;
      const int cnt = mol_popc(adj & M);
      int u = 0;
      for (int c = 0; c < n; ++c) {                             // bounded by n: some atom of M has c < n unmatched neighbours
        const uint64_t at = __ballot(in && cnt == c);
        if (at) { u = mol_lowest(at); break; }
      }
      u = __builtin_amdgcn_readfirstlane(u);
      const uint64_t allowed = back ? mol_above(mol_lowest(back & ~((uint64_t)1 << u))) : ~(uint64_t)0;
      const uint64_t cand = readlane_u64(adj, u) & M & allowed;
      if (cand == 0) {                                          // back: the last pair returns, u goes on above its partner
        if (depth == 0) { code = kMolhNoKekule; break; }
        --depth;
        back = __ballot(my_depth == depth);
        M |= back;
        my_depth = my_depth == depth ? -1 : my_depth;
        continue;
      }
      if (made == max_steps) { code = kMolhUndecided; break; }
      const int v = mol_lowest(cand);
      ++made;
      if (lane == u || lane == v) my_depth = depth, my_partner = 1 + (lane == u ? v : u);
      ++depth;
      M &= ~((uint64_t)1 << u | (uint64_t)1 << v);
      back = 0;
    }
  }
  if (lane < L) {
    out_h[lane] = (uint8_t)h;
    out_p[lane] = (code == kMolhOk && ((W >> lane) & 1u)) ? (uint8_t)my_partner : (uint8_t)0;
  }
  if (lane == 0) verdict[row] = (uint8_t)code, atom[row] = first_over;
}

}  // namespace mdt

// ------------------------------------------------------------------------------------------------
// C ABI entry point of this translation unit (declared in include/mdt_hip.h)
// ------------------------------------------------------------------------------------------------
extern "C" int mdt_mol_hydrogens(const int32_t* natoms, const uint32_t* atoms, const int32_t* nbonds, const uint32_t* bonds, int32_t L,
                                 int32_t R, int32_t max_steps, uint8_t* hydrogens, uint8_t* partner, uint8_t* verdict, int32_t* atom,
                                 int32_t* formula, void* stream) {
  if (R < 0) return mdt_bad("mdt_mol_hydrogens: need R >= 0");
  if (L < 1 || L > mdt::kMolMaxL) return mdt_bad("mdt_mol_hydrogens: need 1 <= L <= 64");
  if (max_steps < 1 || max_steps > mdt::kMolhMaxSteps) return mdt_bad("mdt_mol_hydrogens: need 1 <= max_steps <= 4096");
  if (R == 0) return 0;
  if (!natoms || !atoms || !nbonds || !bonds || !hydrogens || !partner || !verdict || !atom || !formula)
    return mdt_bad("mdt_mol_hydrogens: null pointer");
  const unsigned blocks = (unsigned)(((int64_t)R + mdt::kMolhRowsPerBlock - 1) / mdt::kMolhRowsPerBlock);
  hipLaunchKernelGGL(mdt::k_mol_hydrogens, dim3(blocks), dim3(64 * mdt::kMolhRowsPerBlock), 0, (hipStream_t)stream, natoms, atoms,
                     nbonds, bonds, L, R, max_steps, hydrogens, partner, verdict, atom, formula);
  return mdt_finish("mdt_mol_hydrogens");
}
