// The canonical order of csrc/mdt_molcanon.h (molc_row: what k_mol_canon computes) on the HOST, against rows written by
// tools/molcanon_host_rows.py from the Python reference -- meant to be built with AddressSanitizer and UBSan, so that every array
// the functions touch has exactly the size the definition gives it:
//
//   python tools/molcanon_host_rows.py rows.txt
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -I include \
//         tools/molcanon_host_check.cpp -o molcanon_host_check && ./molcanon_host_check rows.txt
//
// Input, whitespace separated: "T L n nb atoms_present bonds_present" and the atom words and bond words actually present for a row;
// "Q t flags nodes" and L priority words, L canon_atoms words, L canon_bonds words: the reference's mdt_mol_canon for row t (nodes
// -1: any value above the cap).  Every answer is asked twice: with input and output arrays of exactly the row's size, and of one
// more (whose last element must come back untouched).  No device is touched.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../moleculediffusiontransformer_amd/csrc/mdt_molcanon.h"
#include "mol_host_graph.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  std::vector<Graph> rows;
  char tag[8];
  long asked = 0, wrong = 0, by_flag[3] = {0}, most = 0, one = 0;
  while (fscanf(f, "%7s", tag) == 1) {
    if (!strcmp(tag, "T")) {
      Graph g;
      if (!read_graph(f, g)) return 2;
      rows.push_back(std::move(g));
    } else if (!strcmp(tag, "Q")) {
      int t, want_flags, want_nodes;
      if (fscanf(f, "%d %d %d", &t, &want_flags, &want_nodes) != 3 || t < 0 || t >= (int)rows.size()) return 2;
      const Graph& g = rows[t];
      const int L = g.width;
      std::vector<unsigned long long> want(3 * L);
      for (unsigned long long& w : want)
        if (fscanf(f, "%llu", &w) != 1) return 2;
      for (int more = 0; more < 2; ++more) {                      // exact sizes, then one more: a touch past the row is a report
        uint32_t* atoms = new uint32_t[g.have_atoms + more];
        uint32_t* bonds = new uint32_t[g.have_bonds + more];
        uint64_t* priority = new uint64_t[L + more];
        uint32_t* canon_atoms = new uint32_t[L + more];
        uint32_t* canon_bonds = new uint32_t[L + more];
        for (int i = 0; i < g.have_atoms; ++i) atoms[i] = g.atoms[i];
        for (int i = 0; i < g.have_bonds; ++i) bonds[i] = g.bonds[i];
        if (more) atoms[g.have_atoms] = bonds[g.have_bonds] = canon_atoms[L] = canon_bonds[L] = 0xFFFFFFFFu, priority[L] = 0xA5A5A5A5A5A5A5A5ull;
        memset(priority, 0xEE, sizeof(uint64_t) * L);
        memset(canon_atoms, 0xEE, sizeof(uint32_t) * L);
        memset(canon_bonds, 0xEE, sizeof(uint32_t) * L);
        int32_t nodes = -7;
        const int got = mdt::molc_row(atoms, bonds, g.n, g.nb, L, priority, canon_atoms, canon_bonds, nodes);
        bool bad = got != want_flags || (want_nodes < 0 ? nodes <= mdt::kMolcMaxNodes : nodes != want_nodes);
        for (int a = 0; a < L; ++a) bad = bad || priority[a] != want[a] || canon_atoms[a] != want[L + a] || canon_bonds[a] != want[2 * L + a];
        if (more) bad = bad || priority[L] != 0xA5A5A5A5A5A5A5A5ull || canon_atoms[L] != 0xFFFFFFFFu || canon_bonds[L] != 0xFFFFFFFFu;
        if (bad) {
          ++wrong;
          fprintf(stderr, "row %d (+%d): flags %d nodes %d, expected %d %d\n", t, more, got, (int)nodes, want_flags, want_nodes);
        }
        delete[] atoms;
        delete[] bonds;
        delete[] priority;
        delete[] canon_atoms;
        delete[] canon_bonds;
      }
      if (want_flags < 0 || want_flags > 2) return 2;
      ++by_flag[want_flags];
      if (want_nodes > most) most = want_nodes;
      one += want_nodes == 1;
      ++asked;
    } else {
      return 2;
    }
  }
  fclose(f);
  printf("%zu rows, %ld canonical orders asked twice (%ld canonical, %ld undecided, %ld no molecule; %ld with one node, at most %ld "
         "nodes), %ld wrong\n",
         rows.size(), asked, by_flag[1], by_flag[2], by_flag[0], one, most, wrong);
  return wrong ? 1 : 0;
}
