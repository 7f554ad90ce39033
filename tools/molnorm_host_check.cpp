// The Kekule view, the pi electrons, the two rings of an entry and the normal form of csrc/mdt_molnorm.h (moln_row: what
// k_mol_normalize computes) on the HOST, against rows written by tools/molnorm_host_rows.py from the Python reference -- meant to be
// built with AddressSanitizer and UBSan, so that every array the functions touch has exactly the size the definition gives it:
//
//   python tools/molnorm_host_rows.py rows.txt
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -I include \
//         tools/molnorm_host_check.cpp -o molnorm_host_check && ./molnorm_host_check rows.txt
//
// Input, whitespace separated: "T L n nb atoms_present bonds_present verdict" and the atom words, bond words, hydrogens, partner
// words and ring sizes actually present for a row, then "A t flags" followed by L atom words and L bond words: the reference's
// answer for row t.  Every answer is asked twice: with input and output arrays of exactly the row's size, and of one more (whose
// last element must come back untouched).  No device is touched.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../moleculediffusiontransformer_amd/csrc/mdt_molnorm.h"
#include "mol_host_graph.h"

struct Row : Graph {
  int verdict;
  std::vector<uint8_t> hydrogens, partner, bond_ring;
};

static bool bytes(FILE* f, std::vector<uint8_t>& to) {
  for (uint8_t& b : to) {
    unsigned v;
    if (fscanf(f, "%u", &v) != 1) return false;
    b = (uint8_t)v;
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  std::vector<Row> rows;
  char tag[8];
  long asked = 0, wrong = 0, normalized = 0, aromatic = 0, changed = 0;
  while (fscanf(f, "%7s", tag) == 1) {
    if (!strcmp(tag, "T")) {
      Row g;
      if (!read_graph(f, g, &g.verdict)) return 2;
      g.hydrogens.resize(g.have_atoms);
      g.partner.resize(g.have_atoms);
      g.bond_ring.resize(g.have_bonds);
      if (!bytes(f, g.hydrogens) || !bytes(f, g.partner) || !bytes(f, g.bond_ring)) return 2;
      rows.push_back(std::move(g));
    } else if (!strcmp(tag, "A")) {
      int t, flags;
      if (fscanf(f, "%d %d", &t, &flags) != 2) return 2;
      const Row& g = rows[t];
      const int L = g.width;
      std::vector<unsigned> want(2 * L);
      for (unsigned& w : want)
        if (fscanf(f, "%u", &w) != 1) return 2;
      for (int more = 0; more < 2; ++more) {                      // exact sizes, then one more: a touch past the row is a report
        uint32_t* atoms = new uint32_t[g.have_atoms + more];
        uint32_t* bonds = new uint32_t[g.have_bonds + more];
        uint8_t* hydrogens = new uint8_t[g.have_atoms + more];
        uint8_t* partner = new uint8_t[g.have_atoms + more];
        uint8_t* bond_ring = new uint8_t[g.have_bonds + more];
        uint32_t* out_atoms = new uint32_t[L + more];
        uint32_t* out_bonds = new uint32_t[L + more];
        for (int i = 0; i < g.have_atoms; ++i) atoms[i] = g.atoms[i], hydrogens[i] = g.hydrogens[i], partner[i] = g.partner[i];
        for (int i = 0; i < g.have_bonds; ++i) bonds[i] = g.bonds[i], bond_ring[i] = g.bond_ring[i];
        if (more)
          atoms[g.have_atoms] = bonds[g.have_bonds] = 0xFFFFFFFFu, hydrogens[g.have_atoms] = partner[g.have_atoms] = 0xFF,
          bond_ring[g.have_bonds] = 0xFF, out_atoms[L] = out_bonds[L] = 0xA5A5A5A5u;
        memset(out_atoms, 0xEE, sizeof(uint32_t) * L);
        memset(out_bonds, 0xEE, sizeof(uint32_t) * L);
        const int got = mdt::moln_row(atoms, bonds, hydrogens, partner, g.verdict, bond_ring, g.n, g.nb, L, out_atoms, out_bonds);
        bool bad = got != flags;
        for (int a = 0; a < L; ++a) bad = bad || out_atoms[a] != want[a] || out_bonds[a] != want[L + a];
        if (more) bad = bad || out_atoms[L] != 0xA5A5A5A5u || out_bonds[L] != 0xA5A5A5A5u;
        if (bad) {
          ++wrong;
          fprintf(stderr, "row %d (+%d): flags %d, expected %d\n", t, more, got, flags);
        }
        delete[] atoms;
        delete[] bonds;
        delete[] hydrogens;
        delete[] partner;
        delete[] bond_ring;
        delete[] out_atoms;
        delete[] out_bonds;
      }
      normalized += flags & mdt::kMolnNormalized ? 1 : 0;
      aromatic += flags & mdt::kMolnAromatic ? 1 : 0;
      changed += flags & mdt::kMolnChanged ? 1 : 0;
      ++asked;
    } else {
      return 2;
    }
  }
  fclose(f);
  printf("%zu rows, %ld answers asked twice (%ld normalised, %ld with an aromatic ring, %ld changed), %ld wrong\n", rows.size(), asked,
         normalized, aromatic, changed, wrong);
  return wrong ? 1 : 0;
}
