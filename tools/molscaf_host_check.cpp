// The scaffold of csrc/mdt_molscaf.h (mols_row: what k_mol_scaffold computes) on the HOST, against rows written by
// tools/molscaf_host_rows.py from the Python reference -- meant to be built with AddressSanitizer and UBSan, so that every array the
// functions touch has exactly the size the definition gives it:
//
//   python tools/molscaf_host_rows.py rows.txt
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -I include \
//         tools/molscaf_host_check.cpp -o molscaf_host_check && ./molscaf_host_check rows.txt
//
// Input, whitespace separated: "T L n nb atoms_present bonds_present" and the atom words and bond words actually present for a row,
// then "A t mode natoms nbonds flags" followed by L atom words, L bond words and L atom_map bytes: the reference's answer for row t
// in that mode.  Every answer is asked twice: with input and output arrays of exactly the row's size, and of one more (whose last
// element must come back untouched).  No device is touched.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../moleculediffusiontransformer_amd/csrc/mdt_molscaf.h"
#include "mol_host_graph.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  std::vector<Graph> rows;
  char tag[8];
  long asked = 0, wrong = 0, scaffolds = 0, pruned = 0, most_rounds = 0;
  while (fscanf(f, "%7s", tag) == 1) {
    if (!strcmp(tag, "T")) {
      Graph g;
      if (!read_graph(f, g)) return 2;
      rows.push_back(std::move(g));
    } else if (!strcmp(tag, "A")) {
      int t, mode, want_n, want_nb, flags;
      if (fscanf(f, "%d %d %d %d %d", &t, &mode, &want_n, &want_nb, &flags) != 5) return 2;
      const Graph& g = rows[t];
      const int L = g.width;
      std::vector<unsigned> want(3 * L);
      for (unsigned& w : want)
        if (fscanf(f, "%u", &w) != 1) return 2;
      for (int more = 0; more < 2; ++more) {                      // exact sizes, then one more: a touch past the row is a report
        uint32_t* atoms = new uint32_t[g.have_atoms + more];
        uint32_t* bonds = new uint32_t[g.have_bonds + more];
        uint32_t* out_atoms = new uint32_t[L + more];
        uint32_t* out_bonds = new uint32_t[L + more];
        uint8_t* atom_map = new uint8_t[L + more];
        for (int i = 0; i < g.have_atoms; ++i) atoms[i] = g.atoms[i];
        for (int i = 0; i < g.have_bonds; ++i) bonds[i] = g.bonds[i];
        if (more)
          atoms[g.have_atoms] = bonds[g.have_bonds] = 0xFFFFFFFFu, out_atoms[L] = out_bonds[L] = 0xA5A5A5A5u, atom_map[L] = 0xA5;
        memset(out_atoms, 0xEE, sizeof(uint32_t) * L);
        memset(out_bonds, 0xEE, sizeof(uint32_t) * L);
        memset(atom_map, 0xEE, L);
        int got_n = -1, got_nb = -1, rounds = -1;
        const int got = mdt::mols_row(atoms, bonds, g.n, g.nb, L, mode, out_atoms, out_bonds, atom_map, got_n, got_nb, rounds);
        bool bad = got != flags || got_n != want_n || got_nb != want_nb;
        for (int a = 0; a < L; ++a) bad = bad || out_atoms[a] != want[a] || out_bonds[a] != want[L + a] || atom_map[a] != want[2 * L + a];
        if (more) bad = bad || out_atoms[L] != 0xA5A5A5A5u || out_bonds[L] != 0xA5A5A5A5u || atom_map[L] != 0xA5;
        if (bad) {
          ++wrong;
          fprintf(stderr, "row %d mode %d (+%d): flags %d natoms %d nbonds %d, expected %d %d %d\n", t, mode, more, got, got_n, got_nb,
                  flags, want_n, want_nb);
        }
        if (rounds > most_rounds) most_rounds = rounds;
        delete[] atoms;
        delete[] bonds;
        delete[] out_atoms;
        delete[] out_bonds;
        delete[] atom_map;
      }
      scaffolds += flags & mdt::kMolsScaffold ? 1 : 0;
      pruned += (flags & mdt::kMolsScaffold) && !(flags & mdt::kMolsWhole) ? 1 : 0;
      ++asked;
    } else {
      return 2;
    }
  }
  fclose(f);
  printf("%zu rows, %ld answers asked twice (%ld with a scaffold, %ld of them pruned, at most %ld rounds), %ld wrong\n", rows.size(), asked,
         scaffolds, pruned, most_rounds, wrong);
  return wrong ? 1 : 0;
}
