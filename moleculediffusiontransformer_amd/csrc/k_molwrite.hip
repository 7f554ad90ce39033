// Graph rows back to token rows on gfx950: a visiting priority per atom that does not depend on the numbering (k_mol_rank), and the
// writer that spells graph arrays as SMILES tokens (k_mol_write), on the graph arrays of k_mol_graph, k_mol_normalize or
// k_mol_scaffold.  The definition -- the root of a component, what may be written, the two passes, the ring numbers, the atom text,
// the bond symbol, the flags, token_atom -- is written out at mdt_mol_rank and mdt_mol_write in include/mdt_hip.h; the per-word
// helpers, the tokens of one atom and the serial forms are mdt_molwrite.h's, which a host program runs.
//
// k_mol_rank: k_mol_key's launch -- one wave per row, LANE = ROOT, the lab and acc columns in LDS as [atom][lane] -- and its
// mol_root_hash, unchanged.  After it lane r holds H_r and column r holds lab_r.  Then LANE = ATOM: the adjacency words from one
// pass over the wave-uniform entries, the components by k_mol_rings' flood (one ballot a level), per component one butterfly
// minimum of H over its lanes and one ballot for the lowest lane that has it, and one read of that column by the component's
// lanes.  Bounded by nb and n.
//
// k_mol_write: one wave per row, four rows (waves) per workgroup, no workgroup barrier.
//   LANE = ATOM   the words, what is not writable (one ballot), the rank of the atom by (priority, index): n wave-uniform compares.
//   LANE = RANK   the adjacency words in rank space from one pass over the entries, so that "the next neighbour in key order" is a
//                 find-first-set.  Pass 1 is a scalar walk: the current atom's word is one readlane pair; a step visits the lowest
//                 neighbour not yet visited or steps back to the parent: at most 2 n steps.  The visited lane keeps its seq and its
//                 parent.
//   LANE = SEQ    pass 1's order is pass 2's (mdt_molwrite.h), so every lane now owns one atom of the output: its neighbours and
//                 their orders from one more pass over the entries, its children from n readlanes, the closures that close and open
//                 at it as two words.  The ring numbers are the second scalar walk, over the atoms and their closures: the number
//                 of closure k lives in lane k.  Then every lane counts the tokens of its atom, one prefix sum over the wave places
//                 them, every lane leaves its tokens in the row's LDS line (class byte and owner), and the wave writes the row out,
//                 the lanes from T up to W writing the zeros, so no word is written twice.
// EVERY LOOP IS BOUNDED BY n, nb OR W.  No dynamically indexed register array: 0 bytes of scratch.  Vector stores only.
#include "mdt_kernels.h"
#include "mdt_device.h"
#include "mdt_molwrite.h"
#include "../../include/mdt_hip.h"

namespace mdt {

constexpr int kMolwRowsPerBlock = 4;                           // waves (rows) of a workgroup
static_assert(kMolwWritten == MDT_MOLW_WRITTEN && kMolwNoFit == MDT_MOLW_NO_FIT && kMolwNoVocabulary == MDT_MOLW_NO_VOCABULARY &&
                  kMolwNotWritable == MDT_MOLW_NOT_WRITABLE && kMolwMaxW == MDT_MOLW_MAX_WIDTH,
              "mdt_hip.h and mdt_molwrite.h agree");

__device__ __forceinline__ uint64_t molw_shfl64(uint64_t v, int lane) {          // lane: any lane's own choice, 0..63
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, lane, 64);
  const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), lane, 64);
  return (uint64_t)hi << 32 | lo;
}

__global__ __launch_bounds__(64) void k_mol_rank(const int32_t* __restrict__ natoms, const uint32_t* __restrict__ atoms,
                                                 const int32_t* __restrict__ nbonds, const uint32_t* __restrict__ bonds, int L,
                                                 uint64_t* __restrict__ priority) {
  extern __shared__ uint64_t s_cols[];                          // lab [L][64], acc [L][64]
  const int64_t row = blockIdx.x;
  const int lane = threadIdx.x;
  const int n = natoms[row], nb = nbonds[row];
  const uint32_t* row_atoms = atoms + row * L;
  const uint32_t* row_bonds = bonds + row * L;
  uint64_t* out = priority + row * L;
  if (!mol_graph_ok_wave(row_bonds, n, nb, L, lane)) {          // the rule of k_mol_key: such a row is no molecule
    if (lane < L) out[lane] = 0;
    return;
  }
  uint64_t* lab = s_cols + lane;
  uint64_t* acc = s_cols + (size_t)L * 64 + lane;
  const uint64_t h = mol_root_hash(row_atoms, row_bonds, n, nb, lane, lab, acc, 64);
  wave_lds_sync();                                              // the columns are read across lanes below
  // ---- lane = atom: its neighbours in the ring graph (bounded by nb <= L) ----
  const uint64_t adj = mol_ring_adj_wave(row_bonds, nb, lane);
  // ---- per component: the root with the smallest (H, index), and its column (at most n floods of at most n levels in all) ----
  const uint64_t all = mol_all(n);
  uint64_t seen = 0, mine = 0;
  while (seen != all) {
    const uint64_t members = mol_component_wave(adj, all, seen);
    const bool member = mol_in(members, lane);
    uint64_t least = member ? h : ~(uint64_t)0;
    for (int off = 32; off >= 1; off >>= 1) {
      const uint64_t other = shfl_xor_u64(least, off);
      least = other < least ? other : least;
    }
    const int root = mol_lowest(__ballot(member && h == least));   // (not empty: some member has the minimum)
    if (member) mine = s_cols[(size_t)lane * 64 + root];       // lab_root[lane]
    seen |= members;
  }
  if (lane < L) out[lane] = lane < n ? mine : 0;
}

__global__ __launch_bounds__(64 * kMolwRowsPerBlock) void k_mol_write(
    const int32_t* __restrict__ natoms, const uint32_t* __restrict__ atoms, const int32_t* __restrict__ nbonds,
    const uint32_t* __restrict__ bonds, const uint64_t* __restrict__ priority, int L, int R, const uint8_t* __restrict__ class_id, int W,
    int32_t* __restrict__ tokens, int32_t* __restrict__ length, uint8_t* __restrict__ token_atom, uint8_t* __restrict__ flags) {
  __shared__ uint64_t s_open[kMolwRowsPerBlock][64];            // by seq: the closures that open there
  __shared__ uint8_t s_atom[kMolwRowsPerBlock][64];             // by seq: the atom's index in the row
  __shared__ uint8_t s_par[kMolwRowsPerBlock][64];              // by seq: the parent's seq
  __shared__ uint8_t s_base[kMolwRowsPerBlock][64];             // by seq: the slot of its first opening closure
  __shared__ uint8_t s_number[kMolwRowsPerBlock][64];           // by slot: the ring number
  __shared__ uint8_t s_cls[kMolwRowsPerBlock][kMolwMaxW];       // the row's line: class bytes,
  __shared__ uint8_t s_own[kMolwRowsPerBlock][kMolwMaxW];       // and token_atom
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t row = (int64_t)blockIdx.x * kMolwRowsPerBlock + wave;
  if (row >= R) return;                                         // (a whole wave leaves; nothing below crosses waves)
  const int n = natoms[row], nb = nbonds[row];
  const uint32_t* row_bonds = bonds + row * L;
  int32_t* out_t = tokens + row * W;                            // lane and lane + 64 < W <= 128: the whole row, two stores of the wave
  uint8_t* out_a = token_atom + row * W;
  // a row without tokens: every word 0, the length and the flags as given
  auto nothing = [&](int len, int f) {
    for (int j = lane; j < W; j += 64) out_t[j] = 0, out_a[j] = 0;
    if (lane == 0) length[row] = len, flags[row] = (uint8_t)f;
  };
  if (!mol_graph_ok_wave(row_bonds, n, nb, L, lane)) {          // the rule of k_mol_key: such a row is no molecule
    nothing(0, 0);
    return;
  }
  // ---- lane = atom, lane = entry: what is not writable; the ring graph for the entries named twice (bounded by nb <= L) ----
  const bool here = lane < n;                                   // (n, nb <= L <= 64 from here on)
  const uint32_t d = here ? atoms[row * L + lane] : 0u;
  const uint32_t my_word = lane < nb ? row_bonds[lane] : (uint32_t)1 << 16 | 1u << 8;   // (beyond nb: a harmless (0, 1, 1))
  bool bad = (here && !molw_atom_ok(d)) || mol_a(my_word) == mol_b(my_word) || !mol_order_ok(mol_order(my_word));
  uint64_t adj = 0;
  for (int e = 0; e < nb; ++e) {
    const uint32_t w = row_bonds[e];                            // the same word in every lane
    const int a = mol_a(w), b = mol_b(w);
    const uint64_t far = (a == lane ? (uint64_t)1 << b : 0) | (b == lane ? (uint64_t)1 << a : 0);
    bad = bad || (adj & far) != 0;
    adj |= far;
  }
  if (__any(bad)) {
    nothing(0, kMolwNotWritable);
    return;
  }
  // ---- the rank of every atom by (priority, index): n wave-uniform compares ----
  const uint64_t p = (priority != nullptr && here) ? priority[row * L + lane] : 0;
  int rank = 0;
  for (int x = 0; x < n; ++x) {
    const uint64_t px = readlane_u64(p, x);
    rank += (px < p || (px == p && x < lane)) ? 1 : 0;
  }
  rank = here ? rank : lane;                                    // (a permutation of all 64 lanes: the lanes beyond n stay)
  // ---- lane = rank: the adjacency words in rank space ----
  uint64_t adj_rank = 0;
  for (int e = 0; e < nb; ++e) {
    const uint32_t w = row_bonds[e];
    const int ra = readlane_i32(rank, mol_a(w)), rb = readlane_i32(rank, mol_b(w));
    adj_rank |= (lane == ra ? (uint64_t)1 << rb : 0) | (lane == rb ? (uint64_t)1 << ra : 0);
  }
  // ---- pass 1: the scalar walk (at most 2 n steps: a step visits an atom or steps back) ----
  const uint64_t all = mol_all(n);
  uint64_t visited = 0;
  int count = 0, my_seq = lane, my_par = kMolwRoot, my_par_rank = 0;           // (lane = rank; beyond n a lane keeps itself)
  while (visited != all) {
    const int root = mol_lowest(all & ~visited);
    int cur = root, cur_seq = count;
    if (lane == cur) my_seq = count, my_par = kMolwRoot;
    visited |= (uint64_t)1 << cur;
    ++count;
    for (;;) {
      const uint64_t cand = readlane_u64(adj_rank, cur) & ~visited;
      if (cand != 0) {
        const int next = mol_lowest(cand);
        if (lane == next) my_seq = count, my_par = cur_seq, my_par_rank = cur;
        visited |= (uint64_t)1 << next;
        cur = next, cur_seq = count;
        ++count;
      } else if (cur == root) {
        break;
      } else {
        const int up = readlane_i32(my_par_rank, cur);
        cur_seq = readlane_i32(my_par, cur);
        cur = up;
      }
    }
  }
  // ---- lane = seq: the atom of every seq and its parent (through LDS), its word, its neighbours and their orders ----
  const int seq_of_atom = __shfl(my_seq, rank, 64);             // lane = atom: the seq of the lane that holds its rank
  s_par[wave][my_seq] = (uint8_t)my_par;                        // (lane = rank; my_seq is a permutation of the 64 lanes)
  s_atom[wave][seq_of_atom] = (uint8_t)lane;                    // (lane = atom)
  wave_lds_sync();
  MolwAtom me;
  me.atom = s_atom[wave][lane];
  me.par = here ? (int)s_par[wave][lane] : kMolwRoot;
  me.d = (uint32_t)__shfl((int)d, me.atom, 64);
  me.adj = me.o0 = me.o1 = me.o2 = me.child = 0;
  for (int e = 0; e < nb; ++e) {
    const uint32_t w = row_bonds[e];
    const int sa = readlane_i32(seq_of_atom, mol_a(w)), sb = readlane_i32(seq_of_atom, mol_b(w)), o = mol_order(w);
    const uint64_t far = (lane == sa ? (uint64_t)1 << sb : 0) | (lane == sb ? (uint64_t)1 << sa : 0);
    me.adj |= far, me.o0 |= (o & 1) ? far : 0, me.o1 |= (o & 2) ? far : 0, me.o2 |= (o & 4) ? far : 0;
  }
  for (int t = 0; t < n; ++t)                                   // the children: every atom tells its parent
    me.child |= readlane_i32(me.par, t) == lane ? (uint64_t)1 << t : 0;
  const uint64_t aromatic = __ballot(here && (me.d & kMolAromatic) != 0);
  const uint64_t my_open = here ? me.opens(lane) : 0, my_close = here ? me.closes(lane) : 0;
  int base = mol_popc(my_open);                                // -> the exclusive prefix sum over the lanes
  for (int off = 1; off < 64; off <<= 1) {
    const int below = __shfl_up(base, off, 64);
    base += lane >= off ? below : 0;
  }
  base -= mol_popc(my_open);
  // ---- the ring numbers: the second scalar walk, over the atoms and their closures; lane k keeps the number of slot k ----
  uint64_t free_numbers = ~(uint64_t)0;                         // bit k: number k + 1 (at most 63 closures: never empty)
  int my_number = 0;
  for (int s = 0; s < n; ++s) {
    uint64_t closed = 0;
    for (uint64_t left = readlane_u64(my_close, s); left != 0; left &= left - 1) {
      const int t = mol_lowest(left);
      const int slot = readlane_i32(base, t) + mol_popc(readlane_u64(my_open, t) & mol_below(s));
      closed |= (uint64_t)1 << (readlane_i32(my_number, slot) - 1);
    }
    int slot = readlane_i32(base, s);
    for (uint64_t left = readlane_u64(my_open, s); left != 0; left &= left - 1, ++slot) {
      const int k = mol_lowest(free_numbers);
      free_numbers &= ~((uint64_t)1 << k);
      my_number = lane == slot ? k + 1 : my_number;
    }
    free_numbers |= closed;
  }
  s_open[wave][lane] = my_open;
  s_base[wave][lane] = (uint8_t)base;
  s_number[wave][lane] = (uint8_t)my_number;
  wave_lds_sync();
  // ---- pass 2: every lane counts the tokens of its atom; one prefix sum places them ----
  const uint64_t others = molw_shfl64(me.child, me.par & 63);   // (taken by the whole wave; read only below a parent)
  const uint64_t parent_child = me.par == kMolwRoot ? 0 : others;
  MolwSink out = {class_id, nullptr, nullptr, W, 0, false};
  if (here) molw_atom_tokens(me, lane, parent_child, aromatic, s_atom[wave], s_open[wave], s_base[wave], s_number[wave], out);
  const int mine = out.pos;
  int end = mine;                                               // -> the inclusive prefix sum over the lanes
  for (int off = 1; off < 64; off <<= 1) {
    const int below = __shfl_up(end, off, 64);
    end += lane >= off ? below : 0;
  }
  const int T = __builtin_amdgcn_readlane(end, 63);
  if (__any(out.missing)) {
    nothing(T, kMolwNoVocabulary);
    return;
  }
  if (T > W) {
    nothing(T, kMolwNoFit);
    return;
  }
  out.cls = s_cls[wave], out.own = s_own[wave], out.pos = end - mine;
  if (here) molw_atom_tokens(me, lane, parent_child, aromatic, s_atom[wave], s_open[wave], s_base[wave], s_number[wave], out);
  wave_lds_sync();
  for (int j = lane; j < W; j += 64) {                          // (T <= W: every position below T was left by one lane)
    out_t[j] = j < T ? (int32_t)class_id[s_cls[wave][j]] : 0;
    out_a[j] = j < T ? s_own[wave][j] : (uint8_t)0;
  }
  if (lane == 0) length[row] = T, flags[row] = (uint8_t)kMolwWritten;
}

}  // namespace mdt

// ------------------------------------------------------------------------------------------------
// C ABI entry points of this translation unit (declared in include/mdt_hip.h)
// ------------------------------------------------------------------------------------------------
extern "C" int mdt_mol_rank(const int32_t* natoms, const uint32_t* atoms, const int32_t* nbonds, const uint32_t* bonds, int32_t L,
                            int32_t R, uint64_t* priority, void* stream) {
  if (R < 0) return mdt_bad("mdt_mol_rank: need R >= 0");
  if (L < 1 || L > mdt::kMolMaxL) return mdt_bad("mdt_mol_rank: need 1 <= L <= 64");
  if (R == 0) return 0;
  if (!natoms || !atoms || !nbonds || !bonds || !priority) return mdt_bad("mdt_mol_rank: null pointer");
  hipLaunchKernelGGL(mdt::k_mol_rank, dim3((unsigned)R), dim3(64), (size_t)2 * L * 64 * sizeof(uint64_t), (hipStream_t)stream, natoms,
                     atoms, nbonds, bonds, L, priority);
  return mdt_finish("mdt_mol_rank");
}

extern "C" int mdt_mol_write(const int32_t* natoms, const uint32_t* atoms, const int32_t* nbonds, const uint32_t* bonds,
                             const uint64_t* priority, int32_t L, int32_t R, const uint8_t* class_id, int32_t W, int32_t* tokens,
                             int32_t* length, uint8_t* token_atom, uint8_t* flags, void* stream) {
  if (R < 0) return mdt_bad("mdt_mol_write: need R >= 0");
  if (L < 1 || L > mdt::kMolMaxL) return mdt_bad("mdt_mol_write: need 1 <= L <= 64");
  if (W < 1 || W > mdt::kMolwMaxW) return mdt_bad("mdt_mol_write: need 1 <= W <= 128");
  if (R == 0) return 0;
  if (!natoms || !atoms || !nbonds || !bonds || !class_id || !tokens || !length || !token_atom || !flags)
    return mdt_bad("mdt_mol_write: null pointer");
  const unsigned blocks = (unsigned)(((int64_t)R + mdt::kMolwRowsPerBlock - 1) / mdt::kMolwRowsPerBlock);
  hipLaunchKernelGGL(mdt::k_mol_write, dim3(blocks), dim3(64 * mdt::kMolwRowsPerBlock), 0, (hipStream_t)stream, natoms, atoms, nbonds,
                     bonds, priority, L, R, class_id, W, tokens, length, token_atom, flags);
  return mdt_finish("mdt_mol_write");
}
