// The per-atom rule, the matching search and the formula of csrc/mdt_molh.h (molh_row: what k_mol_hydrogens computes) on the HOST,
// against rows written by tools/molh_host_rows.py from the Python reference -- meant to be built with AddressSanitizer and UBSan, so
// that every array the functions touch has exactly the size the definition gives it:
//
//   python tools/molh_host_rows.py rows.txt
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -I include \
//         tools/molh_host_check.cpp -o molh_host_check && ./molh_host_check rows.txt
//
// Input, whitespace separated: "T L n nb atoms_present bonds_present" and the atom and bond words actually present for a row, then
// "H t max_steps verdict atom steps" followed by L hydrogens, L partners and 13 formula words: the reference's answer for row t
// under that cap.  Every answer is asked twice: with input and output arrays of exactly the row's size, and of one more (whose last
// element must come back untouched).  No device is touched.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../moleculediffusiontransformer_amd/csrc/mdt_molh.h"
#include "mol_host_graph.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  std::vector<Graph> rows;
  char tag[8];
  long asked = 0, wrong = 0, steps_max = 0, by_verdict[4] = {0, 0, 0, 0};
  while (fscanf(f, "%7s", tag) == 1) {
    if (!strcmp(tag, "T")) {
      Graph g;
      if (!read_graph(f, g)) return 2;
      rows.push_back(std::move(g));
    } else if (!strcmp(tag, "H")) {
      int t, cap, verdict, atom, steps;
      if (fscanf(f, "%d %d %d %d %d", &t, &cap, &verdict, &atom, &steps) != 5) return 2;
      const Graph& g = rows[t];
      const int L = g.width;
      std::vector<int> want(2 * L + mdt::kMolhFormula);
      for (int& w : want)
        if (fscanf(f, "%d", &w) != 1) return 2;
      for (int more = 0; more < 2; ++more) {                      // exact sizes, then one more: a touch past the row is a report
        uint32_t* atoms = new uint32_t[g.have_atoms + more];
        uint32_t* bonds = new uint32_t[g.have_bonds + more];
        uint8_t* hydrogens = new uint8_t[L + more];
        uint8_t* partner = new uint8_t[L + more];
        int32_t* formula = new int32_t[mdt::kMolhFormula + more];
        for (int i = 0; i < g.have_atoms; ++i) atoms[i] = g.atoms[i];
        for (int i = 0; i < g.have_bonds; ++i) bonds[i] = g.bonds[i];
        if (more) atoms[g.have_atoms] = bonds[g.have_bonds] = 0xFFFFFFFFu, hydrogens[L] = partner[L] = 0xA5, formula[mdt::kMolhFormula] = -77;
        memset(hydrogens, 0xEE, L);
        memset(partner, 0xEE, L);
        for (int k = 0; k < mdt::kMolhFormula; ++k) formula[k] = -99;
        int got_atom = 12345, got_steps = -1;
        const int got = mdt::molh_row(atoms, bonds, g.n, g.nb, L, cap, hydrogens, partner, formula, got_atom, got_steps);
        bool bad = got != verdict || got_atom != atom || got_steps != steps;
        for (int a = 0; a < L; ++a) bad = bad || hydrogens[a] != want[a] || partner[a] != want[L + a];
        for (int k = 0; k < mdt::kMolhFormula; ++k) bad = bad || formula[k] != want[2 * L + k];
        if (more) bad = bad || hydrogens[L] != 0xA5 || partner[L] != 0xA5 || formula[mdt::kMolhFormula] != -77;
        if (bad) {
          ++wrong;
          fprintf(stderr, "row %d cap %d (+%d): verdict %d atom %d steps %d, expected %d %d %d\n", t, cap, more, got, got_atom,
                  got_steps, verdict, atom, steps);
        }
        delete[] atoms;
        delete[] bonds;
        delete[] hydrogens;
        delete[] partner;
        delete[] formula;
      }
      steps_max = steps > steps_max ? steps : steps_max;
      if (verdict >= 0 && verdict < 4) ++by_verdict[verdict];
      ++asked;
    } else {
      return 2;
    }
  }
  fclose(f);
  printf("%zu rows, %ld answers asked twice (verdict 0: %ld, 1: %ld, 2: %ld, 3: %ld), most steps of a row %ld, %ld wrong\n", rows.size(),
         asked, by_verdict[0], by_verdict[1], by_verdict[2], by_verdict[3], steps_max, wrong);
  return wrong ? 1 : 0;
}
