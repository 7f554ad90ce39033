// The walk of csrc/mdt_molmcs.h (mcs_pair, mcs_root_walk, mcs_root_greedy: the code k_mol_mcs runs) on the HOST, against rows
// written by tools/molmcs_host_rows.py from the Python reference -- meant to be built with AddressSanitizer and UBSan, so that every
// array the functions touch has exactly the size the definition gives it:
//
//   python tools/molmcs_host_rows.py rows.txt
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -I include \
//         tools/molmcs_host_check.cpp -o molmcs_host_check && ./molmcs_host_check rows.txt
//
// Input, whitespace separated: "G L n nb atoms_present bonds_present" and the atom and bond words actually present (arrays of
// exactly that size are handed over), then "P a b mode bonds atoms bond_a steps flags out_natoms out_nbonds floor", LA map bytes,
// LA atom words, LA bond words, LA atom_map bytes, "roots" and "a0 b0 size steps capped" for every root.  No device is touched.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../moleculediffusiontransformer_amd/csrc/mdt_molmcs.h"
#include "mol_host_graph.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  std::vector<Graph> graphs;
  char tag[8];
  long pairs = 0, roots = 0, wrong = 0, steps_max = 0, with_cap = 0, steps_all = 0;
  while (fscanf(f, "%7s", tag) == 1) {
    if (!strcmp(tag, "G")) {
      Graph g;
      if (!read_graph(f, g)) return 2;                            // exact sizes: a read past the counts is a report
      graphs.push_back(std::move(g));
    } else if (!strcmp(tag, "P")) {
      int ia, ib, mode, want_bonds, want_atoms, want_steps, want_flags, want_natoms, want_nbonds, want_floor, count;
      unsigned long long want_mask;
      if (fscanf(f, "%d %d %d %d %d %llu %d %d %d %d %d", &ia, &ib, &mode, &want_bonds, &want_atoms, &want_mask, &want_steps,
                 &want_flags, &want_natoms, &want_nbonds, &want_floor) != 11)
        return 2;
      const Graph &a = graphs[ia], &b = graphs[ib];
      const int LA = a.width;
      const bool both = a.n >= 1 && a.n <= a.width && b.n >= 1 && b.n <= b.width;
      const int cells = both ? a.n * b.n : 1;
      uint8_t *map_a = new uint8_t[LA], *atom_map = new uint8_t[LA], *root_capped = new uint8_t[cells];   // exactly LA words each
      uint32_t *out_atoms = new uint32_t[LA], *out_bonds = new uint32_t[LA];
      int *root_size = new int[cells], *root_steps = new int[cells];
      int32_t size[2], steps, out_natoms, out_nbonds;
      uint64_t bond_a;
      uint8_t flags;
      int floor;
      mdt::mcs_pair(a.atoms.get(), a.bonds.get(), a.n, a.nb, LA, b.atoms.get(), b.bonds.get(), b.n, b.nb, b.width, mode, size, map_a, &bond_a, &steps,
                    &out_natoms, out_atoms, &out_nbonds, out_bonds, atom_map, &flags, root_size, root_steps, root_capped, &floor);
      bool bad = size[0] != want_bonds || size[1] != want_atoms || bond_a != want_mask || steps != want_steps || flags != want_flags ||
                 out_natoms != want_natoms || out_nbonds != want_nbonds || floor != want_floor;
      for (int part = 0; part < 4; ++part)
        for (int i = 0; i < LA; ++i) {
          unsigned word;
          if (fscanf(f, "%u", &word) != 1) return 2;
          bad = bad || word != (part == 0 ? map_a[i] : part == 1 ? out_atoms[i] : part == 2 ? out_bonds[i] : atom_map[i]);
        }
      if (fscanf(f, "%d", &count) != 1) return 2;
      for (int i = 0; i < count; ++i) {
        int a0, b0, its_size, made, cut;
        if (fscanf(f, "%d %d %d %d %d", &a0, &b0, &its_size, &made, &cut) != 5) return 2;
        const bool inside = (flags & mdt::kMcsPair) && a0 >= 0 && a0 < a.n && b0 >= 0 && b0 < b.n;
        bad = bad || !inside;
        if (inside) {
          const int at = a0 * b.n + b0;
          bad = bad || root_size[at] != its_size || root_steps[at] != made || root_capped[at] != cut;
        }
        steps_max = made > steps_max ? made : steps_max;
      }
      if (bad) {
        ++wrong;
        fprintf(stderr, "pair %d %d mode %d: size %d %d mask %llx steps %d flags %d floor %d, expected %d %d %llx %d %d %d\n", ia, ib, mode,
                size[0], size[1], (unsigned long long)bond_a, steps, flags, floor, want_bonds, want_atoms, want_mask, want_steps,
                want_flags, want_floor);
      }
      with_cap += (flags & mdt::kMcsUndecided) != 0;
      steps_all += steps;
      roots += count;
      ++pairs;
      delete[] map_a;
      delete[] atom_map;
      delete[] root_capped;
      delete[] out_atoms;
      delete[] out_bonds;
      delete[] root_size;
      delete[] root_steps;
    } else {
      return 2;
    }
  }
  fclose(f);
  printf("%zu graphs, %ld pairs (%ld with a capped root), %ld roots, %ld steps, most steps of a root %ld, %ld wrong\n", graphs.size(),
         pairs, with_cap, roots, steps_all, steps_max, wrong);
  return wrong ? 1 : 0;
}
