// The writer of csrc/mdt_molwrite.h (molw_rank_row and molw_row: what k_mol_rank and k_mol_write compute) on the HOST, against rows
// written by tools/molwrite_host_rows.py from the Python reference -- meant to be built with AddressSanitizer and UBSan, so that every
// array the functions touch has exactly the size the definition gives it:
//
//   python tools/molwrite_host_rows.py rows.txt
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -I include \
//         tools/molwrite_host_check.cpp -o molwrite_host_check && ./molwrite_host_check rows.txt
//
// Input, whitespace separated: "C v" and the 128 class_id bytes of vocabulary v; "T L n nb atoms_present bonds_present" and the atom
// words and bond words actually present for a row; "P t" and L priority words: the reference's mdt_mol_rank for row t; "A t v
// invariant W length flags" followed by W tokens and W token_atom bytes: the reference's mdt_mol_write for row t under vocabulary v,
// with that priority or without one.  Every answer is asked twice: with input and output arrays of exactly the row's size, and of
// one more (whose last element must come back untouched).  No device is touched.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../moleculediffusiontransformer_amd/csrc/mdt_molwrite.h"
#include "mol_host_graph.h"

struct Row : Graph {
  std::vector<uint64_t> priority;
};

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  std::vector<Row> rows;
  std::vector<std::vector<uint8_t>> tables;
  char tag[8];
  long ranked = 0, asked = 0, wrong = 0, by_flag[9] = {0}, longest = 0;
  while (fscanf(f, "%7s", tag) == 1) {
    if (!strcmp(tag, "C")) {
      int v;
      if (fscanf(f, "%d", &v) != 1 || v != (int)tables.size()) return 2;
      std::vector<uint8_t> table(mdt::kMolwClasses);
      for (uint8_t& c : table) {
        unsigned x;
        if (fscanf(f, "%u", &x) != 1) return 2;
        c = (uint8_t)x;
      }
      tables.push_back(table);
    } else if (!strcmp(tag, "T")) {
      Row g;
      if (!read_graph(f, g)) return 2;
      rows.push_back(std::move(g));
    } else if (!strcmp(tag, "P")) {
      int t;
      if (fscanf(f, "%d", &t) != 1) return 2;
      Row& g = rows[t];
      const int L = g.width;
      g.priority.resize(L);
      for (uint64_t& w : g.priority) {
        unsigned long long x;
        if (fscanf(f, "%llu", &x) != 1) return 2;
        w = x;
      }
      for (int more = 0; more < 2; ++more) {                      // exact sizes, then one more: a touch past the row is a report
        uint32_t* atoms = new uint32_t[g.have_atoms + more];
        uint32_t* bonds = new uint32_t[g.have_bonds + more];
        uint64_t* priority = new uint64_t[L + more];
        for (int i = 0; i < g.have_atoms; ++i) atoms[i] = g.atoms[i];
        for (int i = 0; i < g.have_bonds; ++i) bonds[i] = g.bonds[i];
        if (more) atoms[g.have_atoms] = bonds[g.have_bonds] = 0xFFFFFFFFu, priority[L] = 0xA5A5A5A5A5A5A5A5ull;
        memset(priority, 0xEE, sizeof(uint64_t) * L);
        mdt::molw_rank_row(atoms, bonds, g.n, g.nb, L, priority);
        bool bad = more && priority[L] != 0xA5A5A5A5A5A5A5A5ull;
        for (int a = 0; a < L; ++a) bad = bad || priority[a] != g.priority[a];
        if (bad) {
          ++wrong;
          fprintf(stderr, "row %d (+%d): priority differs\n", t, more);
        }
        delete[] atoms;
        delete[] bonds;
        delete[] priority;
      }
      ++ranked;
    } else if (!strcmp(tag, "A")) {
      int t, v, invariant, W, want_length, want_flags;
      if (fscanf(f, "%d %d %d %d %d %d", &t, &v, &invariant, &W, &want_length, &want_flags) != 6) return 2;
      const Row& g = rows[t];
      const int L = g.width;
      std::vector<int> want(2 * W);
      for (int& w : want)
        if (fscanf(f, "%d", &w) != 1) return 2;
      const int have_priority = g.n >= 0 && g.n <= L ? g.n : 0;  // the priority words a molecule row reads: its atoms'
      for (int more = 0; more < 2; ++more) {
        uint32_t* atoms = new uint32_t[g.have_atoms + more];
        uint32_t* bonds = new uint32_t[g.have_bonds + more];
        uint64_t* priority = new uint64_t[have_priority + more];
        uint8_t* class_id = new uint8_t[mdt::kMolwClasses];
        int32_t* tokens = new int32_t[W + more];
        uint8_t* token_atom = new uint8_t[W + more];
        for (int i = 0; i < g.have_atoms; ++i) atoms[i] = g.atoms[i];
        for (int i = 0; i < g.have_bonds; ++i) bonds[i] = g.bonds[i];
        for (int i = 0; i < have_priority; ++i) priority[i] = g.priority[i];
        for (int i = 0; i < mdt::kMolwClasses; ++i) class_id[i] = tables[v][i];
        if (more) atoms[g.have_atoms] = bonds[g.have_bonds] = 0xFFFFFFFFu, priority[have_priority] = 0, tokens[W] = (int32_t)0xA5A5A5A5, token_atom[W] = 0xA5;
        memset(tokens, 0xEE, sizeof(int32_t) * W);
        memset(token_atom, 0xEE, W);
        int got_length = -1;
        const int got = mdt::molw_row(atoms, bonds, invariant ? priority : nullptr, g.n, g.nb, L, class_id, W, tokens, token_atom, got_length);
        bool bad = got != want_flags || got_length != want_length;
        for (int j = 0; j < W; ++j) bad = bad || tokens[j] != want[j] || token_atom[j] != want[W + j];
        if (more) bad = bad || tokens[W] != (int32_t)0xA5A5A5A5 || token_atom[W] != 0xA5;
        if (bad) {
          ++wrong;
          fprintf(stderr, "row %d vocabulary %d invariant %d W %d (+%d): flags %d length %d, expected %d %d\n", t, v, invariant, W, more, got,
                  got_length, want_flags, want_length);
        }
        delete[] atoms;
        delete[] bonds;
        delete[] priority;
        delete[] class_id;
        delete[] tokens;
        delete[] token_atom;
      }
      if (want_flags < 0 || want_flags > 8) return 2;
      ++by_flag[want_flags];
      if (want_length > longest) longest = want_length;
      ++asked;
    } else {
      return 2;
    }
  }
  fclose(f);
  printf("%zu rows, %ld priorities and %ld written rows asked twice (%ld written, %ld too long, %ld without vocabulary, %ld not writable, "
         "%ld no molecule; longest %ld tokens), %ld wrong\n",
         rows.size(), ranked, asked, by_flag[1], by_flag[2], by_flag[4], by_flag[8], by_flag[0], longest, wrong);
  return wrong ? 1 : 0;
}
