// The canonical atom order of graph rows on gfx950 (k_mol_canon), on the graph arrays of k_mol_graph, k_mol_normalize or
// k_mol_scaffold: an individualisation-refinement search over the refinement of k_mol_key, the smallest relabelled graph as the
// answer.  The definition -- refinement with marks, the twin classes, the target of a node, the certificate of a leaf, the order of
// the components, the node cap, the flags -- is written out at mdt_mol_canon in include/mdt_hip.h; the refinement, the twin key, the
// target and the serial form are mdt_molcanon.h's, which a host program runs.
//
// One wave per row.  The search visits the tree BATCH BY BATCH: the children of one node, at most 64, are refined at once, LANE =
// CHILD (the child that marks atom a sits in lane a), the lab and acc columns in LDS as [atom][lane] as k_mol_rank lays them out --
// but L lanes wide, not 64: a child is an atom, so no lane from L up ever has a column, and at L = 32 the row takes 24 KiB of LDS
// where 64-lane columns took 40 (6 rows a CU, not 3).  The root of a component is a batch of one.  Every lane then finds the target
// of its child from its own column (molc_target).
// The leaves of the batch are certified one after the other by the whole wave: LANE = ATOM takes its position by counting the
// smaller (label, index) of the leaf's column, LANE = ENTRY its entry word and its rank among the entries, the certificate goes to
// an LDS line, one ballot per 64 words finds the first difference against the best one, which is kept in LDS behind the best
// certificates of the components already done.  The targets of the children that are no leaves are kept per level in LDS
// ([level][lane], L * L words), the children still to visit per level in a register (LANE = LEVEL), the marks of the path in LDS; the
// next batch is that of the lowest pending child of the deepest level that has one.  After the last component LANE = COMPONENT ranks
// the components by one wave-wide compare per pair, and LANE = ATOM writes the row out.
// EVERY LOOP IS BOUNDED BY n, nb, 64 OR THE NODE CAP (a batch counts its nodes before it refines them).  No dynamically indexed
// register array: 0 bytes of scratch.  Vector stores only.
#include "mdt_kernels.h"
#include "mdt_device.h"
#include "mdt_molcanon.h"
#include "../../include/mdt_hip.h"

namespace mdt {

static_assert(kMolcCanonical == MDT_MOLC_CANONICAL && kMolcUndecided == MDT_MOLC_UNDECIDED && kMolcMaxNodes == MDT_MOLC_MAX_NODES,
              "mdt_hip.h and mdt_molcanon.h agree");

// dynamic LDS of a row of width L: the lab and acc columns [L][L], the targets per level [L][L]
__host__ __device__ inline size_t molc_lds_bytes(int L) { return (size_t)3 * L * L * sizeof(uint64_t); }

__global__ __launch_bounds__(64) void k_mol_canon(const int32_t* __restrict__ natoms, const uint32_t* __restrict__ atoms,
                                                  const int32_t* __restrict__ nbonds, const uint32_t* __restrict__ bonds, int L,
                                                  uint64_t* __restrict__ priority, uint32_t* __restrict__ canon_atoms,
                                                  uint32_t* __restrict__ canon_bonds, int32_t* __restrict__ nodes,
                                                  uint8_t* __restrict__ flags) {
  extern __shared__ uint64_t s_cols[];                          // lab [L][L], acc [L][L], targets [L][L]
  __shared__ uint64_t s_twins[64];                              // by atom: its twins
  __shared__ uint32_t s_best[kMolcCertAll];                     // the best certificate of every component, one behind the other
  __shared__ uint32_t s_cand[kMolcCertOne];                     // the certificate of the leaf in hand
  __shared__ uint8_t s_marks[64];                               // the marks of the path
  const int64_t row = blockIdx.x;
  const int lane = threadIdx.x;
  const int n = natoms[row], nb = nbonds[row];
  const uint32_t* row_atoms = atoms + row * L;
  const uint32_t* row_bonds = bonds + row * L;
  uint64_t* out_p = priority + row * L;
  uint32_t* out_a = canon_atoms + row * L;
  uint32_t* out_b = canon_bonds + row * L;
  // a row without an order: every word 0, the count and the flags as given
  auto nothing = [&](int f, int count) {
    if (lane < L) out_p[lane] = 0, out_a[lane] = 0, out_b[lane] = 0;
    if (lane == 0) nodes[row] = count, flags[row] = (uint8_t)f;
  };
  if (!mol_graph_ok_wave(row_bonds, n, nb, L, lane)) {          // the rule of k_mol_key: such a row is no molecule
    nothing(0, 0);
    return;
  }
  uint64_t* lab = s_cols + lane;                                // (the lanes below L: the others have no column and never refine)
  uint64_t* acc = s_cols + (size_t)L * L + lane;
  uint64_t* s_target = s_cols + (size_t)2 * L * L;
  // ---- lane = atom: its word, its neighbours in the ring graph, its twins; lane = entry: its word (bounded by nb and n) ----
  const bool here = lane < n;                                   // (n, nb <= L <= 64 from here on)
  const uint32_t d = here ? row_atoms[lane] : 0u;
  const uint32_t my_word = lane < nb ? row_bonds[lane] : 0u;
  uint64_t adj = 0;                                             // (mol_ring_adj_wave's loop, kept here: through the helper the
  for (int e = 0; e < nb; ++e) {                                //  kernel came out with 60 VGPRs where this spelling gives 56)
    const uint32_t w = row_bonds[e];                            // the same word in every lane
    const int a = mol_a(w), b = mol_b(w);
    if (a != b) adj |= (a == lane ? mol_bit(b) : 0) | (b == lane ? mol_bit(a) : 0);
  }
  const uint64_t twin_key = here ? molc_twin_key(row_bonds, nb, lane) : 0;
  uint64_t twins = 0;
  for (int b = 0; b < n; ++b) {
    const uint64_t kb = readlane_u64(twin_key, b);
    const uint32_t db = (uint32_t)readlane_i32((int)d, b);
    twins |= (twin_key != 0 && kb == twin_key && db == d) ? (uint64_t)1 << b : 0;
  }
  s_twins[lane] = twins;
  wave_lds_sync();
  // ---- the components, one search each ----
  const uint64_t all = mol_all(n);
  uint64_t seen = 0;
  int count = 0, used = 0, components = 0;                      // wave-uniform: the nodes, the words of s_best in use
  int my_pos = 0, my_component = 0;                             // lane = atom: its position in the best leaf; its component
  int c_start = 0, c_size = 0, c_inside = 0;                    // lane = component: its certificate in s_best, its atoms and entries
  while (seen != all) {                                         // at most n floods of at most n levels in all
    const uint64_t members = mol_component_wave(adj, all, seen);
    seen |= members;
    const bool member = mol_in(members, lane);
    const int size = mol_popc(members);
    const bool mine_in = lane < nb && mol_in(members, mol_a(my_word));   // lane = entry: inside this component
    const uint64_t inside_mask = __ballot(mine_in);
    const int inside = mol_popc(inside_mask), words = 2 + size + inside;
    uint32_t* best = s_best + used;                             // (used + words <= kMolcCertAll: the sizes and the counts sum to <= 64 each)
    bool have = false;
    int level = 0;                                              // the batch in hand: nodes of `level` marks
    uint64_t kids = 1, marked = 0, my_pending = 0;              // its lanes (the root: lane 0); the marks of the path; lane = level
    for (;;) {                                                  // a turn counts at least one node: bounded by the node cap
      count += mol_popc(kids);
      if (count > kMolcMaxNodes) {
        nothing(kMolcUndecided, count);
        return;
      }
      const bool active = mol_in(kids, lane);
      if (lane < L)
        molc_refine(row_atoms, row_bonds, n, nb, s_marks, level > 0 ? level - 1 : 0, (level > 0 && active) ? lane : kMolcNoMark, lab, acc, L);
      const uint64_t open = members & ~marked & ~(level > 0 ? (uint64_t)1 << lane : 0);
      const uint64_t target = active ? molc_target(lab, L, n, open, s_twins) : 0;   // (active: a lane below n)
      if (lane < L) s_target[level * L + lane] = target;        // (level <= n - 1: a node of v marks has a parent with 2 atoms unmarked)
      wave_lds_sync();                                          // the columns are read across lanes below
      const uint64_t inner = __ballot(active && target != 0);
      // ---- the leaves of the batch, one after the other: lane = atom, lane = entry ----
      for (uint64_t left = kids & ~inner; left != 0; left &= left - 1) {
        const int leaf = mol_lowest(left);
        const uint64_t key = here ? s_cols[(size_t)lane * L + leaf] : 0;
        int pos = 0;
        for (int x = 0; x < n; ++x) {
          const uint64_t kx = s_cols[(size_t)x * L + leaf];     // the same word in every lane
          pos += (mol_in(members, x) && (kx < key || (kx == key && x < lane))) ? 1 : 0;
        }
        const int pa = __shfl(pos, mol_a(my_word), 64), pb = __shfl(pos, mol_b(my_word), 64);
        const uint32_t entry = molc_entry(pa, pb, mol_order(my_word));
        int rank = 0;
        for (int x = 0; x < nb; ++x) {
          const uint32_t ex = (uint32_t)readlane_i32((int)entry, x);
          rank += (mol_in(inside_mask, x) && (ex < entry || (ex == entry && x < lane))) ? 1 : 0;
        }
        if (member) s_cand[1 + pos] = d;
        if (mine_in) s_cand[2 + size + rank] = entry;
        if (lane == 0) s_cand[0] = (uint32_t)size, s_cand[1 + size] = (uint32_t)inside;
        wave_lds_sync();
        bool better = !have, decided = !have;
        for (int base = 0; base < words && !decided; base += 64) {
          const int i = base + lane;
          const uint64_t differ = __ballot(i < words && s_cand[i] != best[i]);
          if (differ != 0) {
            const int first = base + mol_lowest(differ);
            better = s_cand[first] < best[first];
            decided = true;
          }
        }
        if (!decided) {                                         // one certificate: the positions in ascending atom index decide
          const uint64_t differ = __ballot(member && pos != my_pos);
          if (differ != 0) better = readlane_i32(pos, mol_lowest(differ)) < readlane_i32(my_pos, mol_lowest(differ));
        }
        if (better) {
          for (int i = lane; i < words; i += 64) best[i] = s_cand[i];
          my_pos = member ? pos : my_pos;
          have = true;
        }
        wave_lds_sync();                                        // the line is written again by the next leaf
      }
      // ---- the next batch: the lowest pending child of the deepest level that has one ----
      uint64_t pend = inner;
      while (pend == 0 && level > 0) {
        --level;
        if (level >= 1) marked &= ~((uint64_t)1 << __builtin_amdgcn_readfirstlane((int)s_marks[level - 1]));
        pend = readlane_u64(my_pending, level);
      }
      if (pend == 0) break;
      const int child = mol_lowest(pend);
      pend &= pend - 1;
      my_pending = lane == level ? pend : my_pending;
      kids = uniform_u64(s_target[level * L + child]);
      if (level >= 1) {
        if (lane == 0) s_marks[level - 1] = (uint8_t)child;
        marked |= (uint64_t)1 << child;
      }
      ++level;
      wave_lds_sync();                                          // the mark is read, the columns are written again
    }
    my_component = member ? components : my_component;
    if (lane == components) c_start = used, c_size = size, c_inside = inside;
    used += words;
    ++components;
  }
  // ---- lane = component: its rank by (certificate, lowest atom) -- they were found in ascending lowest atom ----
  int c_rank = 0;
  for (int i = 0; i < components; ++i) {
    for (int j = i + 1; j < components; ++j) {                  // (bounded by 64 * 63 / 2)
      const int si = readlane_i32(c_start, i), sj = readlane_i32(c_start, j);
      const int wi = 2 + readlane_i32(c_size, i) + readlane_i32(c_inside, i), wj = 2 + readlane_i32(c_size, j) + readlane_i32(c_inside, j);
      const int shorter = wi < wj ? wi : wj;                    // (equal up to the shorter one's end only if equally long: the sizes lead)
      bool j_first = false, decided = false;
      for (int base = 0; base < shorter && !decided; base += 64) {
        const int k = base + lane;
        const uint64_t differ = __ballot(k < shorter && s_best[si + k] != s_best[sj + k]);
        if (differ != 0) {
          const int first = base + mol_lowest(differ);
          j_first = s_best[sj + first] < s_best[si + first];
          decided = true;
        }
      }
      c_rank += (lane == i && j_first) || (lane == j && !j_first) ? 1 : 0;
    }
  }
  int c_offset = 0, c_entries = 0;                              // the atoms and the entries of the components before it
  for (int x = 0; x < components; ++x) {
    const bool before = readlane_i32(c_rank, x) < c_rank;
    c_offset += before ? readlane_i32(c_size, x) : 0;
    c_entries += before ? readlane_i32(c_inside, x) : 0;
  }
  // ---- the row: lane = atom, then per component lane = entry; the lanes from the counts up to L write the zeros ----
  const int my_offset = __shfl(c_offset, my_component, 64);
  if (lane < L) out_p[lane] = here ? (uint64_t)(1 + my_offset + my_pos) : 0;
  if (here) out_a[my_offset + my_pos] = d;                      // (a permutation of 0..n-1: every word is written once)
  else if (lane < L) out_a[lane] = 0;
  for (int c = 0; c < components; ++c) {
    const int start = readlane_i32(c_start, c), size = readlane_i32(c_size, c), inside = readlane_i32(c_inside, c);
    const int offset = readlane_i32(c_offset, c), entries = readlane_i32(c_entries, c);
    if (lane < inside) out_b[entries + lane] = molc_bond_word(s_best[start + 2 + size + lane], offset);
  }
  if (lane >= nb && lane < L) out_b[lane] = 0;                  // (the entries of the components are the nb entries of the row)
  if (lane == 0) nodes[row] = count, flags[row] = (uint8_t)kMolcCanonical;
}

}  // namespace mdt

// ------------------------------------------------------------------------------------------------
// C ABI entry point of this translation unit (declared in include/mdt_hip.h)
// ------------------------------------------------------------------------------------------------
extern "C" int mdt_mol_canon(const int32_t* natoms, const uint32_t* atoms, const int32_t* nbonds, const uint32_t* bonds, int32_t L,
                             int32_t R, uint64_t* priority, uint32_t* canon_atoms, uint32_t* canon_bonds, int32_t* nodes,
                             uint8_t* flags, void* stream) {
  if (R < 0) return mdt_bad("mdt_mol_canon: need R >= 0");
  if (L < 1 || L > mdt::kMolMaxL) return mdt_bad("mdt_mol_canon: need 1 <= L <= 64");
  if (R == 0) return 0;
  if (!natoms || !atoms || !nbonds || !bonds || !priority || !canon_atoms || !canon_bonds || !nodes || !flags)
    return mdt_bad("mdt_mol_canon: null pointer");
  static mdt::DevOnce attr_once;                                // per device (mdt_kernels.h); L = 64: 96 KiB of columns and targets
  if (attr_once.first())
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&mdt::k_mol_canon), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)mdt::molc_lds_bytes(mdt::kMolMaxL));
  hipLaunchKernelGGL(mdt::k_mol_canon, dim3((unsigned)R), dim3(64), mdt::molc_lds_bytes(L), (hipStream_t)stream, natoms, atoms, nbonds,
                     bonds, L, priority, canon_atoms, canon_bonds, nodes, flags);
  return mdt_finish("mdt_mol_canon");
}
