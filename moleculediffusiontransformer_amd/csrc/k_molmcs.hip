// What do these two molecules share?  Maximum common substructure of row pairs on gfx950: per pair (A row, B row) the greatest
// connected common subgraph by (bonds, atoms), edge kind, on the graph arrays of k_mol_graph.  The definition -- the atom and bond
// rules, the roots, the walk of a root with its bound, its floor and its step cap, which is what makes "undecided" a defined answer
// -- is written out at mdt_mol_mcs in include/mdt_hip.h; the walk itself is mdt_molmcs.h's mcs_root_walk, which a host program runs
// as well.
//
// k_mol_mcs: 2 waves per workgroup, ONE WAVE PER PAIR at a time (the waves walk the pairs grid-stride and never meet), LANE = ROOT:
// the na * nb pairs (a0, b0) are taken in ascending rounds of 64, a lane whose pair is incompatible sits its round out.  Two passes
// over the rounds: the greedy descents, whose greatest size is the floor (one LDS atomic max a lane), then the walks under that
// floor.  A lane keeps, over its rounds, the key of its best root (size, then the lower root) and the step at which that best was
// recorded -- not the map: after one LDS atomic max over the lanes the ONE winning lane runs its root's walk again up to that step
// (at most kMcsMaxSteps steps), and the lanes read the map from its bytes.  k_sub_map hands out its first map the same way.
// Per wave in LDS (kMcsWaveBytes): the five adjacency columns of A and of B (2 x 2,560 B, built by the lanes that own an entry with
// 64-bit OR), compat, A's entries per atom, A's entries below each atom (3 x 512 B), A's entries per order (40 B), A's bond words
// (256 B), one dword row for the renumbered outputs (256 B), eight words of results; per lane the map (64 B) and the stack (64 B: a
// level consumes an entry, so 64 levels), each lane-major with a stride of 68 B = 17 dwords, odd, so equal depths of 32 lanes fall
// into 32 banks -- never a register array.  What a level needs on the way back is computed again from the map (mdt_molmcs.h).
// 15,952 B a wave, 31,904 B a workgroup of 2 waves: five workgroups, 10 waves, share a compute unit's 160 KB.  0 bytes of scratch.
// Every loop is bounded by an atom count, an entry count or the cap.  Every output word is written here, by plain vector stores.
#include "mdt_kernels.h"
#include "mdt_device.h"
#include "mdt_molmcs.h"
#include "../../include/mdt_hip.h"

namespace mdt {

constexpr int kMcsRowsPerBlock = 2;                            // waves of a workgroup, one pair each at a time
constexpr int kMcsLaneStride = 68;                             // bytes of one lane's map, and of its stack: 64 and one more dword
constexpr int kMcsMaxBlocks = 2048;                            // 8 workgroups for each of 256 compute units
static_assert(kMcsMaxSteps == MDT_MCS_MAX_STEPS && kMcsExactAtoms == MDT_MCS_EXACT_ATOMS, "mdt_hip.h and mdt_molmcs.h agree");
static_assert(kMcsPair == MDT_MCS_PAIR && kMcsCommon == MDT_MCS_COMMON && kMcsUndecided == MDT_MCS_UNDECIDED &&
                  kMcsWholeA == MDT_MCS_WHOLE_A && kMcsWholeB == MDT_MCS_WHOLE_B,
              "mdt_hip.h and mdt_molmcs.h agree");
static_assert(kMcsLaneStride >= kMolMaxL && (kMcsLaneStride / 4) % 2 == 1, "a map fits and its stride is an odd number of dwords");

struct McsWave {
  unsigned long long adj_a[kMcsOrders * 64], adj_b[kMcsOrders * 64];
  unsigned long long compat[64], at[64], low[64], ord[kMcsOrders];
  unsigned long long total_b, mapped;
  uint32_t ent[64], row[64];
  uint32_t floor, key, steps, capped, winner, pad;
  uint8_t m[64 * kMcsLaneStride], st[64 * kMcsLaneStride];
};
constexpr int kMcsWaveBytes = (int)sizeof(McsWave);
static_assert(kMcsWaveBytes == 15952 && kMcsWaveBytes * kMcsRowsPerBlock <= 64 * 1024, "the LDS budget of the head comment");

__global__ __launch_bounds__(64 * kMcsRowsPerBlock) void k_mol_mcs(
    const int32_t* __restrict__ a_natoms, const uint32_t* __restrict__ a_atoms, const int32_t* __restrict__ a_nbonds,
    const uint32_t* __restrict__ a_bonds, int LA, int R, const int32_t* __restrict__ b_natoms, const uint32_t* __restrict__ b_atoms,
    const int32_t* __restrict__ b_nbonds, const uint32_t* __restrict__ b_bonds, int LB, int RB, int mode, int32_t* __restrict__ size,
    uint8_t* __restrict__ map_a, unsigned long long* __restrict__ bond_a, int32_t* __restrict__ steps, int32_t* __restrict__ out_natoms,
    uint32_t* __restrict__ out_atoms, int32_t* __restrict__ out_nbonds, uint32_t* __restrict__ out_bonds, uint8_t* __restrict__ atom_map,
    uint8_t* __restrict__ flags) {
  __shared__ McsWave s_wave[kMcsRowsPerBlock];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  McsWave& s = s_wave[wave];
  const McsLane l{s.m + lane * kMcsLaneStride, 1, s.st + lane * kMcsLaneStride, 1};
  // ---- the pairs: bounded by R ----
  for (int64_t row = (int64_t)blockIdx.x * kMcsRowsPerBlock + wave; row < R; row += (int64_t)gridDim.x * kMcsRowsPerBlock) {
    const int64_t rb = RB == 1 ? 0 : row;
    const int na = a_natoms[row], nba = a_nbonds[row], nb = b_natoms[rb], nbb = b_nbonds[rb];
    const uint32_t* pa_bonds = a_bonds + row * LA;
    const uint32_t* pb_bonds = b_bonds + rb * LB;
    // the rule of k_mol_key, on either side: such a row is no molecule and the pair no pair
    const bool ok = mol_graph_ok_wave(pa_bonds, na, nba, LA, lane) && mol_graph_ok_wave(pb_bonds, nb, nbb, LB, lane);
    int o_bonds = 0, o_atoms = 0, o_steps = 0, o_flags = 0, image = 0, renum = 0;
    uint64_t matched = 0;
    uint32_t atom_word = 0, bond_word = 0;                      // this lane's words of out_atoms / out_bonds
    if (ok) {                                                   // (wave-uniform)
      o_flags = kMcsPair;
      for (int o = 0; o < kMcsOrders; ++o) s.adj_a[o * 64 + lane] = 0, s.adj_b[o * 64 + lane] = 0;   // bounded by the five orders
      s.at[lane] = 0;
      if (lane < kMcsOrders) s.ord[lane] = 0;
      if (lane == 0) s.total_b = 0, s.mapped = 0, s.floor = 0, s.key = 0, s.steps = 0, s.capped = 0;
      wave_lds_sync();
      const uint32_t wa = lane < nba ? pa_bonds[lane] : 0u, wb = lane < nbb ? pb_bonds[lane] : 0u;   // (nba <= LA, nbb <= LB lanes)
      const bool use_a = lane < nba && mcs_usable(wa), use_b = lane < nbb && mcs_usable(wb);
      s.ent[lane] = wa;
      if (use_a) {                                              // (ends < na <= 64, order in 1..5: inside the columns)
        atomicOr(&s.adj_a[(mol_order(wa) - 1) * 64 + mol_a(wa)], 1ull << mol_b(wa));
        atomicOr(&s.adj_a[(mol_order(wa) - 1) * 64 + mol_b(wa)], 1ull << mol_a(wa));
        atomicOr(&s.at[mol_a(wa)], 1ull << lane);
        atomicOr(&s.at[mol_b(wa)], 1ull << lane);
        atomicOr(&s.ord[mol_order(wa) - 1], 1ull << lane);
      }
      if (use_b) {
        atomicOr(&s.adj_b[(mol_order(wb) - 1) * 64 + mol_a(wb)], 1ull << mol_b(wb));
        atomicOr(&s.adj_b[(mol_order(wb) - 1) * 64 + mol_b(wb)], 1ull << mol_a(wb));
      }
      const uint64_t all = __ballot(use_a);
      const uint32_t da = lane < na ? a_atoms[row * LA + lane] : 0u, db = lane < nb ? b_atoms[rb * LB + lane] : 0u;
      wave_lds_sync();
      uint64_t below = 0;
      for (int a = 0; a < na; ++a) {                            // bounded by na <= LA; wave-uniform
        const uint32_t word = (uint32_t)__shfl((int)da, a);
        const uint64_t accepted = __ballot(lane < nb && mcs_compatible(word, db, mode));
        if (lane == 0) s.compat[a] = accepted;
        if (a < lane) below |= s.at[a];
      }
      s.low[lane] = below;
      for (int o = 0; o < kMcsOrders; ++o) {                    // B's bonds of each order as a set: every pair once, at its lower atom
        const int mine = mol_popc(s.adj_b[o * 64 + lane] & mol_above(lane));
        if (mine) atomicAdd(&s.total_b, (unsigned long long)mine << (8 * o));
      }
      wave_lds_sync();
      const McsTables t{(const uint64_t*)s.adj_b, (const uint64_t*)s.compat, (const uint64_t*)s.at, (const uint64_t*)s.low,
                        (const uint64_t*)s.ord, s.ent, (uint64_t)s.total_b, all, na, nb};
      const int roots = na * nb;                                // (at most 4096)
      // ---- the floor: every root's greedy descent ----
      int reach = 0;
      for (int base = 0; base < roots; base += 64) {            // bounded by na * nb / 64 rounds
        const int k = base + lane, a0 = k / nb, b0 = k - a0 * nb;
        if (k < roots && ((s.compat[a0] >> b0) & 1ull)) {
          const int g = mcs_root_greedy(t, l, a0, b0);          // bounded by the atoms
          reach = g > reach ? g : reach;
        }
      }
      if (reach) atomicMax(&s.floor, (uint32_t)reach);
      wave_lds_sync();
      const int floor = (int)s.floor;
      // ---- the walks.  No root stops or prunes because of another root's progress: only because of the floor ----
      uint32_t key = 0;
      int key_step = 0, made_all = 0;
      bool cut_any = false;
      for (int base = 0; base < roots; base += 64) {
        const int k = base + lane, a0 = k / nb, b0 = k - a0 * nb;
        if (k < roots && ((s.compat[a0] >> b0) & 1ull)) {
          int at_step, made;
          bool cut;
          uint64_t mapped;
          const int best = mcs_root_walk(t, l, a0, b0, floor, -1, at_step, made, cut, mapped);   // bounded by the step cap
          const uint32_t its = mcs_root_key(best, a0, b0);
          if (its > key) key = its, key_step = at_step;
          made_all += made;
          cut_any = cut_any || cut;
        }
      }
      if (key) atomicMax(&s.key, key);
      if (made_all) atomicAdd(&s.steps, (uint32_t)made_all);    // (at most 4096 roots of 4096 steps: no overflow)
      if (cut_any) s.capped = 1;
      wave_lds_sync();
      const uint32_t won = s.key;                               // (wave-uniform)
      o_steps = (int)s.steps;
      if (s.capped) o_flags |= kMcsUndecided;
      if (won) {
        const int id = 4095 - (int)(won & 4095u), a0 = id >> 6, b0 = id & 63;
        if (key == won) {                                       // one lane: the key names the root.  Its walk once more, to the step
          int at_step, made;                                    // at which its best was recorded
          bool cut;
          uint64_t mapped;
          mcs_root_walk(t, l, a0, b0, floor, key_step, at_step, made, cut, mapped);
          s.mapped = mapped;
          s.winner = (uint32_t)lane;
        }
        wave_lds_sync();
        const uint64_t mapped = s.mapped;
        const uint8_t* wm = s.m + s.winner * kMcsLaneStride;    // the winner's map ...
        uint8_t* inv = s.st + s.winner * kMcsLaneStride;        // ... and, in its stack bytes, the inverse of it
        const bool kept = (mapped >> lane) & 1ull;              // (only bits below na are ever set)
        image = kept ? 1 + wm[lane] : 0;
        renum = kept ? 1 + mol_popc(mapped & (mol_bit(lane) - 1)) : 0;   // (mol_index by the lane's own bit, here and below: through
        o_atoms = mol_popc(mapped);                              //  the helper the compiler forms the lane's mask a second way)
        inv[lane] = 255;
        wave_lds_sync();
        if (kept) inv[image - 1] = (uint8_t)lane, s.row[renum - 1] = da;
        wave_lds_sync();
        atom_word = lane < o_atoms ? s.row[lane] : 0u;
        // the recount: every usable A entry between mapped atoms whose image is a B bond of its order
        const bool in = use_a && ((mapped >> mol_a(wa)) & (mapped >> mol_b(wa)) & 1ull) &&
                        ((s.adj_b[(mol_order(wa) - 1) * 64 + wm[mol_a(wa)]] >> wm[mol_b(wa)]) & 1ull);
        matched = __ballot(in);
        o_bonds = mol_popc(matched);
        // B's side: a usable B entry is in the result when A has a usable entry of its order between the partners of its ends
        const int ua = use_b ? inv[mol_a(wb)] : 255, ub = use_b ? inv[mol_b(wb)] : 255;
        const bool b_out = use_b && (ua == 255 || ub == 255 || !((s.adj_a[(mol_order(wb) - 1) * 64 + (ua & 63)] >> (ub & 63)) & 1ull));
        const bool b_miss = __any(b_out);
        wave_lds_sync();                                        // (the atom words are read: the row takes the bond words)
        if (in)
          s.row[mol_popc(matched & (mol_bit(lane) - 1))] = (uint32_t)mol_index(mapped, mol_a(wa)) | (uint32_t)mol_index(mapped, mol_b(wa)) << 8 |
                                            (uint32_t)mol_order(wa) << 16;
        wave_lds_sync();
        bond_word = lane < o_bonds ? s.row[lane] : 0u;
        o_flags |= kMcsCommon;
        if (o_atoms == na && matched == all) o_flags |= kMcsWholeA;
        if (o_atoms == nb && !b_miss) o_flags |= kMcsWholeB;
      }
    }
    if (lane < LA) {                                            // (LA <= 64 lanes own a word of each row)
      map_a[row * LA + lane] = (uint8_t)image;
      atom_map[row * LA + lane] = (uint8_t)renum;
      out_atoms[row * LA + lane] = atom_word;
      out_bonds[row * LA + lane] = bond_word;
    }
    if (lane == 0) {
      size[row * 2] = o_bonds;
      size[row * 2 + 1] = o_atoms;
      bond_a[row] = matched;
      steps[row] = o_steps;
      out_natoms[row] = o_atoms;
      out_nbonds[row] = o_bonds;
      flags[row] = (uint8_t)o_flags;
    }
    wave_lds_sync();                                            // (the next pair writes the tables again)
  }
}

}  // namespace mdt

// ------------------------------------------------------------------------------------------------
// C ABI entry point of this translation unit (declared in include/mdt_hip.h)
// ------------------------------------------------------------------------------------------------
extern "C" int mdt_mol_mcs(const int32_t* a_natoms, const uint32_t* a_atoms, const int32_t* a_nbonds, const uint32_t* a_bonds, int32_t LA,
                           int32_t R, const int32_t* b_natoms, const uint32_t* b_atoms, const int32_t* b_nbonds, const uint32_t* b_bonds,
                           int32_t LB, int32_t RB, int32_t mode, int32_t* size, uint8_t* map_a, uint64_t* bond_a, int32_t* steps,
                           int32_t* out_natoms, uint32_t* out_atoms, int32_t* out_nbonds, uint32_t* out_bonds, uint8_t* atom_map,
                           uint8_t* flags, void* stream) {
  if (R < 0) return mdt_bad("mdt_mol_mcs: need R >= 0");
  if (LA < 1 || LA > mdt::kMolMaxL) return mdt_bad("mdt_mol_mcs: need 1 <= LA <= 64");
  if (LB < 1 || LB > mdt::kMolMaxL) return mdt_bad("mdt_mol_mcs: need 1 <= LB <= 64");
  if (RB != R && RB != 1) return mdt_bad("mdt_mol_mcs: need RB == R (row by row) or RB == 1 (every A row against the one B row)");
  if (mode & ~MDT_MCS_EXACT_ATOMS) return mdt_bad("mdt_mol_mcs: mode may only have MDT_MCS_EXACT_ATOMS (1)");
  if (R == 0) return 0;
  if (!a_natoms || !a_atoms || !a_nbonds || !a_bonds || !b_natoms || !b_atoms || !b_nbonds || !b_bonds || !size || !map_a || !bond_a ||
      !steps || !out_natoms || !out_atoms || !out_nbonds || !out_bonds || !atom_map || !flags)
    return mdt_bad("mdt_mol_mcs: null pointer");
  const int64_t want = ((int64_t)R + mdt::kMcsRowsPerBlock - 1) / mdt::kMcsRowsPerBlock;
  const unsigned blocks = (unsigned)(want < mdt::kMcsMaxBlocks ? want : mdt::kMcsMaxBlocks);
  hipLaunchKernelGGL(mdt::k_mol_mcs, dim3(blocks), dim3(64 * mdt::kMcsRowsPerBlock), 0, (hipStream_t)stream, a_natoms, a_atoms, a_nbonds,
                     a_bonds, LA, R, b_natoms, b_atoms, b_nbonds, b_bonds, LB, RB, mode, size, map_a, (unsigned long long*)bond_a, steps,
                     out_natoms, out_atoms, out_nbonds, out_bonds, atom_map, flags);
  return mdt_finish("mdt_mol_mcs");
}
