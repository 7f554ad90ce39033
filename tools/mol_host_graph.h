// The graph line of the rows that the tools/*_host_check.cpp programs read, "L n nb atoms_present bonds_present <atom words> <bond
// words>" behind its tag, and the one struct it is read into.  The words live in arrays of EXACTLY atoms_present / bonds_present
// elements from new[], so a function under test that reads one word past what the row holds is an AddressSanitizer report -- a
// vector's capacity, or a fixed array of 64, would hide it.
#pragma once

#include <cstdint>
#include <cstdio>
#include <memory>
#include <utility>

struct Graph {
  int width, n, nb, have_atoms, have_bonds;
  std::unique_ptr<uint32_t[]> atoms, bonds;
};

// Reads one graph line from behind its tag.  between, when given, takes one more integer that stands between the five counts and
// the words (molnorm's verdict).  -> false when the line is cut short or a count is negative.
inline bool read_graph(FILE* f, Graph& g, int* between = nullptr) {
  if (fscanf(f, "%d %d %d %d %d", &g.width, &g.n, &g.nb, &g.have_atoms, &g.have_bonds) != 5) return false;
  if (between && fscanf(f, "%d", between) != 1) return false;
  if (g.have_atoms < 0 || g.have_bonds < 0) return false;
  g.atoms.reset(new uint32_t[g.have_atoms]);
  g.bonds.reset(new uint32_t[g.have_bonds]);
  for (int i = 0; i < g.have_atoms; ++i)
    if (fscanf(f, "%u", &g.atoms[i]) != 1) return false;
  for (int i = 0; i < g.have_bonds; ++i)
    if (fscanf(f, "%u", &g.bonds[i]) != 1) return false;
  return true;
}
