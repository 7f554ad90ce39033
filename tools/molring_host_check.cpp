// The ring search, the components and the descriptors of csrc/mdt_molring.h (molr_row: what k_mol_rings computes) on the HOST,
// against rows written by tools/molring_host_rows.py from the Python reference -- meant to be built with AddressSanitizer and UBSan,
// so that every array the functions touch has exactly the size the definition gives it:
//
//   python tools/molring_host_rows.py rows.txt
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -I include \
//         tools/molring_host_check.cpp -o molring_host_check && ./molring_host_check rows.txt
//
// Input, whitespace separated: "T L n nb atoms_present bonds_present" and the atom words, bond words and hydrogens actually present
// for a row, then "A t bounded flag" followed by 16 lo, 16 hi, L bond_ring, L atom_ring and 16 descriptor words: the reference's
// answer for row t (bounded 0: no bounds are handed over).  Every answer is asked twice: with input and output arrays of exactly
// the row's size, and of one more (whose last element must come back untouched).  No device is touched.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../moleculediffusiontransformer_amd/csrc/mdt_molring.h"
#include "mol_host_graph.h"

struct Row : Graph {
  std::vector<uint8_t> hydrogens;
};

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  std::vector<Row> rows;
  char tag[8];
  long asked = 0, wrong = 0, flagged = 0, with_ring = 0, largest = 0;
  while (fscanf(f, "%7s", tag) == 1) {
    if (!strcmp(tag, "T")) {
      Row g;
      if (!read_graph(f, g)) return 2;
      g.hydrogens.resize(g.have_atoms);
      for (int i = 0; i < g.have_atoms; ++i) {
        unsigned h;
        if (fscanf(f, "%u", &h) != 1) return 2;
        g.hydrogens[i] = (uint8_t)h;
      }
      rows.push_back(std::move(g));
    } else if (!strcmp(tag, "A")) {
      int t, bounded, flag;
      if (fscanf(f, "%d %d %d", &t, &bounded, &flag) != 3) return 2;
      const Row& g = rows[t];
      const int L = g.width, D = mdt::kMolrDesc;
      std::vector<long long> want(2 * D + 2 * L + D);
      for (long long& w : want)
        if (fscanf(f, "%lld", &w) != 1) return 2;
      for (int more = 0; more < 2; ++more) {                      // exact sizes, then one more: a touch past the row is a report
        uint32_t* atoms = new uint32_t[g.have_atoms + more];
        uint32_t* bonds = new uint32_t[g.have_bonds + more];
        uint8_t* hydrogens = new uint8_t[g.have_atoms + more];
        int32_t* lo = new int32_t[D + more];
        int32_t* hi = new int32_t[D + more];
        uint8_t* bond_ring = new uint8_t[L + more];
        uint8_t* atom_ring = new uint8_t[L + more];
        int32_t* desc = new int32_t[D + more];
        for (int i = 0; i < g.have_atoms; ++i) atoms[i] = g.atoms[i], hydrogens[i] = g.hydrogens[i];
        for (int i = 0; i < g.have_bonds; ++i) bonds[i] = g.bonds[i];
        for (int k = 0; k < D; ++k) lo[k] = (int32_t)want[k], hi[k] = (int32_t)want[D + k];
        if (more)
          atoms[g.have_atoms] = bonds[g.have_bonds] = 0xFFFFFFFFu, hydrogens[g.have_atoms] = 0xFF, lo[D] = 0x7FFFFFFF, hi[D] = -0x7FFFFFFF,
          bond_ring[L] = atom_ring[L] = 0xA5, desc[D] = -77;
        memset(bond_ring, 0xEE, L);
        memset(atom_ring, 0xEE, L);
        for (int k = 0; k < D; ++k) desc[k] = -99;
        const int got = mdt::molr_row(atoms, bonds, hydrogens, g.n, g.nb, L, bounded ? lo : nullptr, bounded ? hi : nullptr, bond_ring,
                                      atom_ring, desc);
        bool bad = got != flag;
        for (int a = 0; a < L; ++a) bad = bad || bond_ring[a] != want[2 * D + a] || atom_ring[a] != want[2 * D + L + a];
        for (int k = 0; k < D; ++k) bad = bad || desc[k] != want[2 * D + 2 * L + k];
        if (more) bad = bad || bond_ring[L] != 0xA5 || atom_ring[L] != 0xA5 || desc[D] != -77;
        if (bad) {
          ++wrong;
          fprintf(stderr, "row %d bounded %d (+%d): flag %d, expected %d; rings %d largest %d\n", t, bounded, more, got, flag,
                  desc[mdt::kMolrRings], desc[mdt::kMolrLargestRing]);
        }
        delete[] atoms;
        delete[] bonds;
        delete[] hydrogens;
        delete[] lo;
        delete[] hi;
        delete[] bond_ring;
        delete[] atom_ring;
        delete[] desc;
      }
      const long long* d = &want[2 * D + 2 * L];
      flagged += flag;
      if (!bounded) with_ring += d[mdt::kMolrRings] > 0;
      largest = d[mdt::kMolrLargestRing] > largest ? (long)d[mdt::kMolrLargestRing] : largest;
      ++asked;
    } else {
      return 2;
    }
  }
  fclose(f);
  printf("%zu rows (%ld with a ring, largest ring %ld), %ld answers asked twice (%ld flagged), %ld wrong\n", rows.size(), with_ring,
         largest, asked, flagged, wrong);
  return wrong ? 1 : 0;
}
