// Maximum common substructure of a row pair (mdt_hip.h, mdt_mol_mcs): the walk of one root with its step count, the greedy descent
// behind the floor, and the whole pair root after root.  The bond word, "is this a graph row?" and the sets are mdt_molrow.h's.
// Like mdt_molsub.h everything here is __host__ __device__ and touches only the arrays it is handed, so the kernel (k_molmcs.hip:
// tables in LDS, one root per lane) and a host program (tools/molmcs_host_check.cpp: tables in arrays of exactly their size) run
// the same walk.
//
// All state of a root is 64-bit masks, popcounts and a few ints -- no array but the two it is handed: the map (a byte per A atom)
// and the stack (a byte per level).  A level consumes one A entry for good -- included, it has both ends mapped below that level;
// excluded, it is in X -- so there are at most as many levels as usable entries, 64.  A stack byte is the entry, bit 6 once the
// level has moved on to its exclude branch, bit 7 when the end that was free is the entry's b.  Everything else a level needs on
// the way back -- its candidate word, what its assignment added to the count and to B's used bonds -- is computed again from the
// map, as k_sub_match does with its candidate word.
#pragma once

#include <cstdint>
#include <hip/hip_runtime.h>

#include "mdt_molrow.h"

namespace mdt {

constexpr int kMcsMaxSteps = 4096, kMcsOrders = kMolOrders;
constexpr int kMcsExactAtoms = 1;                               // the one mode bit
enum { kMcsPair = 1, kMcsCommon = 2, kMcsUndecided = 4, kMcsWholeA = 8, kMcsWholeB = 16 };

__host__ __device__ __forceinline__ bool mcs_usable(uint32_t w) { return mol_a(w) != mol_b(w) && mol_order_ok(mol_order(w)); }
__host__ __device__ __forceinline__ bool mcs_compatible(uint32_t a, uint32_t b, int mode) {
  return (mode & kMcsExactAtoms) ? a == b : ((a ^ b) & 0x7FFu) == 0;
}

// The tables of one pair, wherever they live.
//   adj_b[(o - 1) * 64 + u]   the B atoms joined to u by a usable entry of order o
//   compat[a]                 the B atoms that A atom a is compatible with
//   at[a]                     the usable A entries with an end at a
//   low[a]                    the usable A entries with an end below a (the entries root (a, .) may not touch)
//   ord[o - 1]                the usable A entries of order o
//   ent[k]                    A's bond words
//   total_b                   byte o - 1: the B bonds of order o, as a set
//   all                       the usable A entries
struct McsTables {
  const uint64_t* adj_b;
  const uint64_t* compat;
  const uint64_t* at;
  const uint64_t* low;
  const uint64_t* ord;
  const uint32_t* ent;
  uint64_t total_b, all;
  int na, nb;
};

// what one root owns: its map (m[a * m_stride], valid where `mapped` has a bit) and its stack
struct McsLane {
  uint8_t* m;
  int m_stride;
  uint8_t* st;
  int st_stride;
};

struct McsState {
  uint64_t mapped, used, par, both, x, live, inb;               // par: entries with exactly one end mapped; both: with both
  int cur;                                                      // inb byte o - 1: the B bonds of order o with both ends used
};

__host__ __device__ __forceinline__ int mcs_size(const McsState& s) { return s.cur << 8 | mol_popc(s.mapped); }

// what M(y) = at adds: the entries at y, not excluded, whose other end is mapped onto a neighbour of `at` by their order (counted),
// and per order the B bonds from `at` into the used atoms (packed).  y is unmapped and `at` unused in s.  Bounded by the entries at y.
__host__ __device__ __forceinline__ void mcs_gain(const McsTables& t, const McsLane& l, const McsState& s, int y, int at, int& gain,
                                                  uint64_t& inb) {
  gain = 0;
  for (uint64_t e = t.at[y] & s.par & ~s.x; e; e &= e - 1) {
    const uint32_t w = t.ent[mol_lowest(e)];
    const int z = mol_a(w) == y ? mol_b(w) : mol_a(w);
    gain += (int)((t.adj_b[(mol_order(w) - 1) * 64 + at] >> l.m[z * l.m_stride]) & 1u);
  }
  inb = 0;
  for (int o = 0; o < kMcsOrders; ++o) inb |= (uint64_t)mol_popc(t.adj_b[o * 64 + at] & s.used) << (8 * o);
}

__host__ __device__ __forceinline__ void mcs_assign(const McsTables& t, const McsLane& l, McsState& s, int y, int at) {
  int gain;
  uint64_t inb;
  mcs_gain(t, l, s, y, at, gain, inb);
  s.cur += gain;
  s.inb += inb;                                                 // (a byte holds at most 64: no carry)
  s.both |= t.at[y] & s.par;
  s.par ^= t.at[y];
  s.mapped |= mol_bit(y);
  s.used |= mol_bit(at);
  l.m[y * l.m_stride] = (uint8_t)at;
}

__host__ __device__ __forceinline__ void mcs_undo(const McsTables& t, const McsLane& l, McsState& s, int y, int at) {
  s.mapped &= ~mol_bit(y);
  s.used &= ~mol_bit(at);
  s.par ^= t.at[y];
  s.both &= ~t.at[y];
  int gain;
  uint64_t inb;
  mcs_gain(t, l, s, y, at, gain, inb);                          // (x is what it was at the assignment: deeper exclusions are undone)
  s.cur -= gain;
  s.inb -= inb;
}

// step 2: the bound as a size, bonds << 8 | atoms
__host__ __device__ __forceinline__ int mcs_bound(const McsTables& t, const McsState& s, uint64_t atoms_from) {
  const uint64_t rem = s.live & ~s.x & ~s.both;
  int ub = s.cur;
  for (int o = 0; o < kMcsOrders; ++o) {
    const int ra = mol_popc(t.ord[o] & rem);
    const int rb = (int)((t.total_b >> (8 * o)) & 255u) - (int)((s.inb >> (8 * o)) & 255u);
    ub += ra < rb ? ra : rb;
  }
  const int have = mol_popc(s.mapped), free_a = mol_popc(atoms_from & ~s.mapped), free_b = t.nb - have;
  return ub << 8 | (have + (free_a < free_b ? free_a : free_b));
}

// step 3: the lowest live entry, not excluded, with exactly one end mapped and a candidate -> entry k, its free end y, the word c.
// Bounded by the entries.
__host__ __device__ __forceinline__ bool mcs_pick(const McsTables& t, const McsLane& l, const McsState& s, int& k, int& y, uint64_t& c) {
  for (uint64_t e = s.par & s.live & ~s.x; e; e &= e - 1) {
    k = mol_lowest(e);
    const uint32_t w = t.ent[k];
    const bool a_mapped = (s.mapped >> mol_a(w)) & 1u;
    const int x = a_mapped ? mol_a(w) : mol_b(w);
    y = a_mapped ? mol_b(w) : mol_a(w);
    c = t.adj_b[(mol_order(w) - 1) * 64 + l.m[x * l.m_stride]] & t.compat[y] & ~s.used;
    if (c) return true;
  }
  return false;
}

__host__ __device__ __forceinline__ void mcs_root_init(const McsTables& t, const McsLane& l, McsState& s, int a0, int b0) {
  s.mapped = mol_bit(a0);
  s.used = mol_bit(b0);
  s.par = t.at[a0];
  s.both = s.x = s.inb = 0;
  s.live = t.all & ~t.low[a0];
  s.cur = 0;
  l.m[a0 * l.m_stride] = (uint8_t)b0;
}

// the A atoms >= a0 (mol_all(na) with the test written as na == 64, na <= 64 here: k_mol_mcs's code as it has been measured)
__host__ __device__ __forceinline__ uint64_t mcs_atoms_from(const McsTables& t, int a0) {
  return (t.na == 64 ? ~(uint64_t)0 : mol_below(t.na)) & ~mol_below(a0);
}

// The greedy descent of root (a0, b0): always the lowest candidate of step 3, no exclusion, no pruning -> the size it reaches.
// Bounded by the atoms: every pass maps one.
__host__ __device__ inline int mcs_root_greedy(const McsTables& t, const McsLane& l, int a0, int b0) {
  McsState s;
  mcs_root_init(t, l, s, a0, b0);
  int k, y;
  uint64_t c;
  while (mcs_pick(t, l, s, k, y, c)) mcs_assign(t, l, s, y, mol_lowest(c));
  return mcs_size(s);
}

// The walk of root (a0, b0) under `floor` (a size).  -> the root's best size; best_step: the step count at which it was recorded
// (the node entered by that step; 0 is the root's own node); steps; capped.  With stop_at >= 0 the walk ends on entering the node
// of step stop_at, with the map of that node in l.m and its atoms in `mapped`: that is how the winning root's map is handed out.
// Every pass of the loop makes a step or takes a level back, so it runs at most 2 * kMcsMaxSteps + 2 times.
__host__ __device__ inline int mcs_root_walk(const McsTables& t, const McsLane& l, int a0, int b0, int floor, int stop_at, int& best_step,
                                             int& steps, bool& capped, uint64_t& mapped) {
  McsState s;
  mcs_root_init(t, l, s, a0, b0);
  const uint64_t atoms_from = mcs_atoms_from(t, a0);
  int best = -1, at_step = 0, made = 0, sp = 0;
  bool cut = false, enter = true;
  for (;;) {
    if (enter) {
      const int size = mcs_size(s);
      if (size > best) best = size, at_step = made;
      if (made == stop_at) break;
      const int ub = mcs_bound(t, s, atoms_from);
      int k, y;
      uint64_t c;
      if (!(ub <= best || ub < floor) && mcs_pick(t, l, s, k, y, c)) {
        if (made == kMcsMaxSteps) { cut = true; break; }
        ++made;
        l.st[sp * l.st_stride] = (uint8_t)(k | (y == mol_b(t.ent[k]) ? 0x80 : 0));   // (sp < the usable entries <= 64)
        ++sp;
        mcs_assign(t, l, s, y, mol_lowest(c));
        continue;
      }
      enter = false;
    }
    if (sp == 0) break;
    const int top = l.st[(sp - 1) * l.st_stride], k = top & 63;
    if (top & 0x40) {                                           // the exclude branch is done: the level is
      s.x &= ~mol_bit(k);
      --sp;
      continue;
    }
    const uint32_t w = t.ent[k];
    const int y = (top & 0x80) ? mol_b(w) : mol_a(w), x = (top & 0x80) ? mol_a(w) : mol_b(w);
    const int last = l.m[y * l.m_stride];
    mcs_undo(t, l, s, y, last);
    const uint64_t c = t.adj_b[(mol_order(w) - 1) * 64 + l.m[x * l.m_stride]] & t.compat[y] & ~s.used & mol_above(last);
    if (made == kMcsMaxSteps) { cut = true; break; }            // (the next candidate and the exclusion each count one step)
    ++made;
    if (c) {
      mcs_assign(t, l, s, y, mol_lowest(c));
    } else {
      l.st[(sp - 1) * l.st_stride] = (uint8_t)(top | 0x40);
      s.x |= mol_bit(k);
    }
    enter = true;
  }
  best_step = at_step;
  steps = made;
  capped = cut;
  mapped = s.mapped;
  return best;
}

// the key by which roots are compared: greater size first, then the LOWER root (a0 * 64 + b0 < 4096)
__host__ __device__ __forceinline__ uint32_t mcs_root_key(int size, int a0, int b0) {
  return (uint32_t)size << 12 | (uint32_t)(4095 - (a0 * 64 + b0));
}

// Fills the tables of a pair of molecules from the graph arrays: adj_b[5 * 64], compat[64], at[64], low[64], ord[5].  Reads
// a_atoms[0:na], a_bonds[0:nba], b_atoms[0:nb], b_bonds[0:nbb] and nothing beyond.  (The kernel builds the same words with a lane
// per entry.)
__host__ __device__ inline void mcs_fill_tables(const uint32_t* a_atoms, const uint32_t* a_bonds, int na, int nba, const uint32_t* b_atoms,
                                                const uint32_t* b_bonds, int nb, int nbb, int mode, uint64_t* adj_b, uint64_t* compat,
                                                uint64_t* at, uint64_t* low, uint64_t* ord, McsTables& t) {
  for (int i = 0; i < kMcsOrders * 64; ++i) adj_b[i] = 0;
  for (int i = 0; i < 64; ++i) compat[i] = at[i] = low[i] = 0;
  for (int o = 0; o < kMcsOrders; ++o) ord[o] = 0;
  for (int e = 0; e < nbb; ++e) {                               // bounded by nbb <= LB
    const uint32_t w = b_bonds[e];
    if (!mcs_usable(w)) continue;
    adj_b[(mol_order(w) - 1) * 64 + mol_a(w)] |= mol_bit(mol_b(w));
    adj_b[(mol_order(w) - 1) * 64 + mol_b(w)] |= mol_bit(mol_a(w));
  }
  uint64_t total = 0, all = 0;
  for (int o = 0; o < kMcsOrders; ++o) {
    int twice = 0;
    for (int u = 0; u < nb; ++u) twice += mol_popc(adj_b[o * 64 + u]);
    total |= (uint64_t)(twice / 2) << (8 * o);
  }
  for (int e = 0; e < nba; ++e) {                               // bounded by nba <= LA
    const uint32_t w = a_bonds[e];
    if (!mcs_usable(w)) continue;
    all |= mol_bit(e);
    at[mol_a(w)] |= mol_bit(e);
    at[mol_b(w)] |= mol_bit(e);
    ord[mol_order(w) - 1] |= mol_bit(e);
  }
  for (int a = 1; a < na; ++a) low[a] = low[a - 1] | at[a - 1];
  for (int a = 0; a < na; ++a)
    for (int b = 0; b < nb; ++b)
      if (mcs_compatible(a_atoms[a], b_atoms[b], mode)) compat[a] |= mol_bit(b);
  t = McsTables{adj_b, compat, at, low, ord, a_bonds, total, all, na, nb};
}

// One pair of mdt_mol_mcs, root after root, in the order the definition is written down.  Writes size[2], map_a[0:LA], *bond_a,
// *steps, *out_natoms, out_atoms[0:LA], *out_nbonds, out_bonds[0:LA], atom_map[0:LA], *flags -- every word -- and, when given,
// root_size / root_steps / root_capped [na * nb] (root (a0, b0) at a0 * nb + b0; -1 / 0 / 0 for a pair that is no root) and *floor.
// Reads a_atoms[0:na], a_bonds[0:nba], b_atoms[0:nb], b_bonds[0:nbb] and nothing beyond.  k_mol_mcs computes the same with one root
// per lane and the tables in LDS.
__host__ __device__ inline void mcs_pair(const uint32_t* a_atoms, const uint32_t* a_bonds, int na, int nba, int LA, const uint32_t* b_atoms,
                                         const uint32_t* b_bonds, int nb, int nbb, int LB, int mode, int32_t* size, uint8_t* map_a,
                                         uint64_t* bond_a, int32_t* steps, int32_t* out_natoms, uint32_t* out_atoms, int32_t* out_nbonds,
                                         uint32_t* out_bonds, uint8_t* atom_map, uint8_t* flags, int* root_size, int* root_steps,
                                         uint8_t* root_capped, int* floor_out) {
  size[0] = size[1] = 0;
  *bond_a = 0;
  *steps = *out_natoms = *out_nbonds = 0;
  *flags = 0;
  for (int i = 0; i < LA; ++i) map_a[i] = atom_map[i] = 0, out_atoms[i] = out_bonds[i] = 0;
  if (floor_out) *floor_out = 0;
  if (!mol_graph_ok(a_bonds, na, nba, LA, false) || !mol_graph_ok(b_bonds, nb, nbb, LB, false)) return;
  if (root_size)
    for (int i = 0; i < na * nb; ++i) root_size[i] = -1, root_steps[i] = 0, root_capped[i] = 0;
  uint64_t adj_b[kMcsOrders * 64], compat[64], at[64], low[64], ord[kMcsOrders];
  uint8_t m[64], st[64];
  McsTables t;
  mcs_fill_tables(a_atoms, a_bonds, na, nba, b_atoms, b_bonds, nb, nbb, mode, adj_b, compat, at, low, ord, t);
  const McsLane l{m, 1, st, 1};
  int fl = 0;
  uint32_t f = *flags = kMcsPair;
  for (int a0 = 0; a0 < na; ++a0)
    for (int b0 = 0; b0 < nb; ++b0)
      if ((compat[a0] >> b0) & 1u) {
        const int g = mcs_root_greedy(t, l, a0, b0);
        fl = g > fl ? g : fl;
      }
  if (floor_out) *floor_out = fl;
  uint32_t win = 0;
  int win_a = -1, win_b = -1, win_step = 0, total = 0;
  for (int a0 = 0; a0 < na; ++a0)
    for (int b0 = 0; b0 < nb; ++b0)
      if ((compat[a0] >> b0) & 1u) {
        int at_step, made;
        bool cut;
        uint64_t mapped;
        const int best = mcs_root_walk(t, l, a0, b0, fl, -1, at_step, made, cut, mapped);
        if (root_size) root_size[a0 * nb + b0] = best, root_steps[a0 * nb + b0] = made, root_capped[a0 * nb + b0] = cut;
        total += made;
        if (cut) f |= kMcsUndecided;
        const uint32_t key = mcs_root_key(best, a0, b0);
        if (key > win) win = key, win_a = a0, win_b = b0, win_step = at_step;
      }
  *steps = total;
  if (win_a < 0) return;
  int at_step, made;
  bool cut;
  uint64_t mapped;
  mcs_root_walk(t, l, win_a, win_b, fl, win_step, at_step, made, cut, mapped);
  uint64_t matched = 0;
  int kept = 0;
  for (int a = 0; a < na; ++a)
    if ((mapped >> a) & 1u) {
      map_a[a] = (uint8_t)(1 + m[a]);
      out_atoms[kept] = a_atoms[a];
      atom_map[a] = (uint8_t)++kept;
    }
  int kb = 0;
  for (int e = 0; e < nba; ++e) {
    const uint32_t w = a_bonds[e];
    if (!mcs_usable(w) || !((mapped >> mol_a(w)) & (mapped >> mol_b(w)) & 1u)) continue;
    if (!((adj_b[(mol_order(w) - 1) * 64 + m[mol_a(w)]] >> m[mol_b(w)]) & 1u)) continue;
    matched |= mol_bit(e);
    out_bonds[kb++] = (uint32_t)(atom_map[mol_a(w)] - 1) | (uint32_t)(atom_map[mol_b(w)] - 1) << 8 | (uint32_t)mol_order(w) << 16;
  }
  size[0] = kb;
  size[1] = kept;
  *bond_a = matched;
  *out_natoms = kept;
  *out_nbonds = kb;
  f |= kMcsCommon;
  if (kept == na && matched == t.all) f |= kMcsWholeA;
  // B's side: every atom used, and every usable entry of B the image of a matched entry -- as a set, so per order the B bonds
  // against the distinct images
  bool whole_b = kept == nb;
  for (int o = 0; o < kMcsOrders && whole_b; ++o) {
    uint64_t img[64];
    for (int u = 0; u < nb; ++u) img[u] = 0;
    for (uint64_t e = matched & ord[o]; e; e &= e - 1) {
      const uint32_t w = a_bonds[mol_lowest(e)];
      img[m[mol_a(w)]] |= mol_bit(m[mol_b(w)]);
      img[m[mol_b(w)]] |= mol_bit(m[mol_a(w)]);
    }
    for (int u = 0; u < nb; ++u) whole_b = whole_b && img[u] == adj_b[o * 64 + u];
  }
  if (whole_b) f |= kMcsWholeB;
  *flags = (uint8_t)f;
}

}  // namespace mdt
