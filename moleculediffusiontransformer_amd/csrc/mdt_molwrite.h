// Graph rows back to token rows (mdt_hip.h, mdt_mol_rank / mdt_mol_write): what may be written, the characters of an atom word, the
// bond symbol, the ring numbers, the tokens that belong to one atom, and the serial forms of both entry points.  The walk is told in
// SEQ SPACE: once pass 1 has numbered the atoms in the order it first reaches them, the emission of pass 2 is that very order, a child
// is a neighbour above its parent, a closure that closes at s is a neighbour below s that is not its parent, one that opens at s a
// neighbour above s that is not its child -- and "ascending seq of the other end" is "ascending bit" of a 64-bit word.  The
// descriptor, the bond accessors, "is this a graph row?", the sets, the ring graph and its components are mdt_molrow.h's, the
// classes and the rooted hash mdt_smiles_scan.h's.  Like those headers everything here is
// __host__ __device__ and touches only the arrays it is handed.  The kernels (k_molwrite.hip: one wave per row, lane = atom, then
// lane = rank, then lane = seq) use the per-word helpers and molw_atom_tokens as they stand and run the walks on wave-uniform words
// where molw_row walks arrays; a host program (tools/molwrite_host_check.cpp: arrays of exactly their size) runs molw_rank_row and
// molw_row.
#pragma once

#include <cstdint>
#include <hip/hip_runtime.h>

#include "mdt_molrow.h"
#include "mdt_smiles_scan.h"

namespace mdt {

enum { kMolwWritten = 1, kMolwNoFit = 2, kMolwNoVocabulary = 4, kMolwNotWritable = 8 };   // the flags: one of them, or 0
constexpr int kMolwMaxW = 128, kMolwClasses = 128;
constexpr int kMolwRoot = 255;                                 // "no parent" in a byte

// may this atom word be written?  H at most 9, charge field at most 18, both letter fields at most 26
__host__ __device__ __forceinline__ bool molw_atom_ok(uint32_t d) {
  return ((d >> 17) & 15u) <= 9u && ((d >> 12) & 31u) <= 18u && (d & 31u) <= 26u && ((d >> 5) & 31u) <= 26u;
}
// the class of the bond symbol an entry of order o (1..5) needs between two atoms, 0: none -- the inverse of mol_bond_order
__host__ __device__ __forceinline__ int molw_bond_class(int o, bool both_aromatic) {
  return ((o == 1 && !both_aromatic) || (o == 5 && both_aromatic)) ? 0 : kClsBond + o - 1;
}
// is the atom written without brackets?  B C N O P S b c n o p s F I Cl Br *, no charge (field 9 or 0), no H, no isotope, bit 11 clear
__host__ __device__ __forceinline__ bool molw_plain(uint32_t d) {
  const int first = (int)(d & 31u), second = (int)((d >> 5) & 31u);
  const bool aromatic = (d & kMolAromatic) != 0;
  const uint32_t charge = (d >> 12) & 31u;
  if ((d & kMolBracket) || !(charge == 9u || charge == 0u) || ((d >> 17) & 15u) != 0u || (d >> 21) != 0u) return false;
  if (second == 0) return first == kMolStar || is_aromatic(first) || (!aromatic && (first == 'F' - 'A' || first == 'I' - 'A'));
  return !aromatic && ((first == 'C' - 'A' && second == 1 + ('l' - 'a')) || (first == 'B' - 'A' && second == 1 + ('r' - 'a')));
}

// Where the tokens go.  put(class, owner) counts every token and notes a class the vocabulary cannot write; with `cls` set it also
// keeps the tokens at positions below W.  Positions start at `pos`.
struct MolwSink {
  const uint8_t* class_id;
  uint8_t* cls;                                                 // [W] class bytes, or nullptr: count only
  uint8_t* own;                                                 // [W] token_atom
  int W, pos;
  bool missing;
  __host__ __device__ __forceinline__ void put(int c, int owner) {
    missing = missing || class_id[c] == 0;
    if (cls != nullptr && pos < W) cls[pos] = (uint8_t)c, own[pos] = (uint8_t)owner;
    ++pos;
  }
};

// a ring number 1..99: one digit, or % and two
__host__ __device__ __forceinline__ void molw_number(int k, int owner, MolwSink& out) {
  if (k < 10) { out.put(kClsDigit + k, owner); return; }
  out.put(kClsPercent, owner);
  out.put(kClsDigit + k / 10, owner);
  out.put(kClsDigit + k % 10, owner);
}

// the characters of one atom word (molw_atom_ok holds)
__host__ __device__ inline void molw_atom_text(uint32_t d, int owner, MolwSink& out) {
  const int first = (int)(d & 31u), second = (int)((d >> 5) & 31u);
  const bool aromatic = (d & kMolAromatic) != 0;
  const bool plain = molw_plain(d);
  if (!plain) {
    out.put(kClsLBracket, owner);
    const int isotope = (int)(d >> 21);                         // at most 2047
    if (isotope >= 1000) out.put(kClsDigit + isotope / 1000, owner);
    if (isotope >= 100) out.put(kClsDigit + isotope / 100 % 10, owner);
    if (isotope >= 10) out.put(kClsDigit + isotope / 10 % 10, owner);
    if (isotope >= 1) out.put(kClsDigit + isotope % 10, owner);
  }
  out.put(first == kMolStar ? kClsStar : (aromatic ? kClsLower : kClsUpper) + first, owner);
  if (second != 0) out.put(kClsLower + second - 1, owner);
  if (plain) return;
  const int h = (int)((d >> 17) & 15u), charge = (int)((d >> 12) & 31u);
  if (h >= 1) out.put(kClsUpper + ('H' - 'A'), owner);
  if (h >= 2) out.put(kClsDigit + h, owner);
  if (charge != 9 && charge != 0) {
    const int size = charge > 9 ? charge - 9 : 9 - charge;
    out.put(charge > 9 ? kClsPlus : kClsMinus, owner);
    if (size >= 2) out.put(kClsDigit + size, owner);
  }
  out.put(kClsRBracket, owner);
}

// What the walks leave for the atom with seq s.  adj: its neighbours (seq space); o0, o1, o2: the bits of the order of the entry
// to each neighbour; par: its parent's seq or kMolwRoot; child: its children; d: its word; atom: its index in the row.
struct MolwAtom {
  uint64_t adj, o0, o1, o2, child;
  uint32_t d;
  int par, atom;
  __host__ __device__ __forceinline__ int order(int t) const { return (int)((o0 >> t) & 1u) | (int)((o1 >> t) & 1u) << 1 | (int)((o2 >> t) & 1u) << 2; }
  __host__ __device__ __forceinline__ uint64_t parent_bit() const { return par == kMolwRoot ? 0 : (uint64_t)1 << par; }
  __host__ __device__ __forceinline__ uint64_t closes(int s) const { return adj & mol_below(s) & ~parent_bit(); }
  __host__ __device__ __forceinline__ uint64_t opens(int s) const { return adj & mol_above(s) & ~child; }
};

// The tokens of the atom with seq s, in order: what stands before it -- '.' before a later root; otherwise ')' when the atom before
// it is not its parent (the branch of its elder sibling ends), '(' when it is not its parent's last child, the bond symbol -- its
// text, the numbers of the closures that close at it, the symbol and number of those that open at it.  parent_child: the children
// of its parent; aromatic: the aromatic atoms (seq space); atom_of[t]: the row index of seq t; open_of[t], base_of[t]: the closures
// that open at t and the slot of the first of them in number_of[].
__host__ __device__ inline void molw_atom_tokens(const MolwAtom& me, int s, uint64_t parent_child, uint64_t aromatic, const uint8_t* atom_of,
                                                 const uint64_t* open_of, const uint8_t* base_of, const uint8_t* number_of,
                                                 MolwSink& out) {
  const int owner = 1 + me.atom;
  const bool arom = mol_in(aromatic, s);
  if (me.par == kMolwRoot) {
    if (s > 0) out.put(kClsDot, 0);
  } else {
    if (me.par != s - 1) out.put(kClsClose, 1 + atom_of[mol_highest(parent_child & mol_below(s))]);
    if ((parent_child & mol_above(s)) != 0) out.put(kClsOpen, owner);
    const int c = molw_bond_class(me.order(me.par), arom && mol_in(aromatic, me.par));
    if (c != 0) out.put(c, owner);
  }
  molw_atom_text(me.d, owner, out);
  for (uint64_t left = me.closes(s); left != 0; left &= left - 1) {           // bounded by n
    const int t = mol_lowest(left);
    molw_number(number_of[base_of[t] + mol_popc(open_of[t] & mol_below(s))], owner, out);
  }
  int slot = base_of[s];
  for (uint64_t left = me.opens(s); left != 0; left &= left - 1, ++slot) {    // bounded by n
    const int t = mol_lowest(left);
    const int c = molw_bond_class(me.order(t), arom && mol_in(aromatic, t));
    if (c != 0) out.put(c, owner);
    molw_number(number_of[slot], owner, out);
  }
}

// mdt_mol_rank of one row.  Reads atoms[0:n], bonds[0:nb]; writes priority[0:L] and nothing beyond.
__host__ __device__ inline void molw_rank_row(const uint32_t* atoms, const uint32_t* bonds, int n, int nb, int L, uint64_t* priority) {
  for (int a = 0; a < L; ++a) priority[a] = 0;
  if (!mol_graph_ok(bonds, n, nb, L, false)) return;
  uint64_t lab[kMolMaxL], acc[kMolMaxL], h[kMolMaxL], adj[kMolMaxL];
  mol_ring_adj(bonds, n, nb, adj);
  for (int r = 0; r < n; ++r) h[r] = mol_root_hash(atoms, bonds, n, nb, r, lab, acc, 1);
  uint64_t seen = 0;
  while (seen != mol_all(n)) {                                 // one component a turn
    const uint64_t members = mol_component(adj, n, seen);
    int root = -1;
    for (int r = 0; r < n; ++r)
      if (mol_in(members, r) && (root < 0 || h[r] < h[root])) root = r;
    mol_root_hash(atoms, bonds, n, nb, root, lab, acc, 1);
    for (int a = 0; a < n; ++a)
      if (mol_in(members, a)) priority[a] = lab[a];
    seen |= members;
  }
}

// mdt_mol_write of one row.  Reads atoms[0:n], bonds[0:nb], priority[0:n] (or nullptr: as numbered), class_id[0:128]; writes
// tokens[0:W], token_atom[0:W] and nothing beyond.  -> the flags; length: the token count T (0 for no molecule and for flags 8).
__host__ __device__ inline int molw_row(const uint32_t* atoms, const uint32_t* bonds, const uint64_t* priority, int n, int nb, int L,
                                        const uint8_t* class_id, int W, int32_t* tokens, uint8_t* token_atom, int& length) {
  for (int j = 0; j < W; ++j) tokens[j] = 0, token_atom[j] = 0;
  length = 0;
  if (!mol_graph_ok(bonds, n, nb, L, false)) return 0;         // (n == 0 included: no molecule)
  uint64_t adj[kMolMaxL];                                       // the ring graph, row numbering
  for (int a = 0; a < n; ++a) adj[a] = 0;
  bool bad = false;
  for (int a = 0; a < n; ++a) bad = bad || !molw_atom_ok(atoms[a]);
  for (int e = 0; e < nb; ++e) {
    const int a = mol_a(bonds[e]), b = mol_b(bonds[e]);
    bad = bad || a == b || mol_in(adj[a], b) || !mol_order_ok(mol_order(bonds[e]));
    adj[a] |= (uint64_t)1 << b, adj[b] |= (uint64_t)1 << a;
  }
  if (bad) return kMolwNotWritable;
  // ---- the rank of every atom by (priority, index), and the graph in rank space ----
  uint8_t rank[kMolMaxL], seq_of_rank[kMolMaxL], seq_of[kMolMaxL];
  for (int a = 0; a < n; ++a) {
    int below = 0;
    for (int x = 0; x < n; ++x) {
      const uint64_t px = priority ? priority[x] : 0, pa = priority ? priority[a] : 0;
      below += (px < pa || (px == pa && x < a)) ? 1 : 0;
    }
    rank[a] = (uint8_t)below;
  }
  uint64_t adj_rank[kMolMaxL];
  for (int a = 0; a < n; ++a) adj_rank[a] = 0;
  for (int e = 0; e < nb; ++e) {
    const int ra = rank[mol_a(bonds[e])], rb = rank[mol_b(bonds[e])];
    adj_rank[ra] |= (uint64_t)1 << rb, adj_rank[rb] |= (uint64_t)1 << ra;
  }
  // ---- pass 1: the depth-first walk; the next atom is the lowest neighbour not yet visited, else the walk steps back ----
  MolwAtom at[kMolMaxL];                                        // by seq
  uint8_t par_rank[kMolMaxL];
  uint64_t visited = 0;
  int count = 0;
  while (visited != mol_all(n)) {                              // bounded by 2 n steps in all: a step visits an atom or steps back
    const int root = mol_lowest(mol_all(n) & ~visited);
    int cur = root;
    seq_of_rank[cur] = (uint8_t)count, at[count].par = kMolwRoot, ++count, visited |= (uint64_t)1 << cur;
    for (;;) {
      const uint64_t cand = adj_rank[cur] & ~visited;
      if (cand != 0) {
        const int next = mol_lowest(cand);
        seq_of_rank[next] = (uint8_t)count, at[count].par = seq_of_rank[cur], par_rank[next] = (uint8_t)cur, ++count;
        visited |= (uint64_t)1 << next;
        cur = next;
      } else if (cur == root) {
        break;
      } else {
        cur = par_rank[cur];
      }
    }
  }
  // ---- the graph in seq space ----
  uint8_t atom_of[kMolMaxL], base_of[kMolMaxL], number_of[kMolMaxL];
  uint64_t open_of[kMolMaxL];
  uint64_t aromatic = 0;
  for (int a = 0; a < n; ++a) {
    const int s = seq_of[a] = seq_of_rank[rank[a]];
    atom_of[s] = (uint8_t)a;
    at[s].adj = at[s].o0 = at[s].o1 = at[s].o2 = at[s].child = 0, at[s].d = atoms[a], at[s].atom = a;
    if (atoms[a] & kMolAromatic) aromatic |= (uint64_t)1 << s;
  }
  for (int e = 0; e < nb; ++e) {
    const int sa = seq_of[mol_a(bonds[e])], sb = seq_of[mol_b(bonds[e])], o = mol_order(bonds[e]);
    for (int side = 0; side < 2; ++side) {
      MolwAtom& x = at[side ? sb : sa];
      const uint64_t far = (uint64_t)1 << (side ? sa : sb);
      x.adj |= far, x.o0 |= (o & 1) ? far : 0, x.o1 |= (o & 2) ? far : 0, x.o2 |= (o & 4) ? far : 0;
    }
  }
  for (int s = 0; s < n; ++s)
    if (at[s].par != kMolwRoot) at[at[s].par].child |= (uint64_t)1 << s;
  // ---- the ring numbers: in seq order, the numbers that close at s are read, those that open at s take the lowest free one,
  //      and what closed at s is free from the next atom on (at most 63 closures: a number is at most 64) ----
  int slots = 0;
  for (int s = 0; s < n; ++s) open_of[s] = at[s].opens(s), base_of[s] = (uint8_t)slots, slots += mol_popc(open_of[s]);
  uint64_t free_numbers = ~(uint64_t)0;                         // bit k: number k + 1
  for (int s = 0; s < n; ++s) {
    uint64_t closed = 0;
    for (uint64_t left = at[s].closes(s); left != 0; left &= left - 1) {
      const int t = mol_lowest(left);
      closed |= (uint64_t)1 << (number_of[base_of[t] + mol_popc(open_of[t] & mol_below(s))] - 1);
    }
    int slot = base_of[s];
    for (uint64_t left = open_of[s]; left != 0; left &= left - 1, ++slot) {
      const int k = mol_lowest(free_numbers);
      free_numbers &= ~((uint64_t)1 << k);
      number_of[slot] = (uint8_t)(k + 1);
    }
    free_numbers |= closed;
  }
  // ---- pass 2: the tokens, counted, then kept where they fit ----
  uint8_t cls[kMolwMaxW], own[kMolwMaxW];
  MolwSink out = {class_id, nullptr, nullptr, W, 0, false};
  for (int round = 0; round < 2; ++round) {
    for (int s = 0; s < n; ++s)
      molw_atom_tokens(at[s], s, at[s].par == kMolwRoot ? 0 : at[at[s].par].child, aromatic, atom_of, open_of, base_of, number_of, out);
    if (round == 1) break;
    length = out.pos;
    if (out.missing) return kMolwNoVocabulary;
    if (length > W) return kMolwNoFit;
    out.cls = cls, out.own = own, out.pos = 0;
  }
  for (int j = 0; j < length; ++j) tokens[j] = (int32_t)class_id[cls[j]], token_atom[j] = own[j];
  return kMolwWritten;
}

}  // namespace mdt
