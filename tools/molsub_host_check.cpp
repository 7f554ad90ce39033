// The substructure search of csrc/mdt_molsub.h (sub_match_pair, sub_root_search: the code k_sub_match runs) on the HOST, against
// rows written by tools/molsub_host_rows.py from the Python reference -- meant to be built with AddressSanitizer and UBSan, so that
// every array the functions touch has exactly the size the definition gives it:
//
//   python tools/molsub_host_rows.py rows.txt
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -I include \
//         tools/molsub_host_check.cpp -o molsub_host_check && ./molsub_host_check rows.txt
//
// Input, whitespace separated: "T L n nb atoms_present bonds_present" and the atom and bond words actually present (arrays of
// exactly that size are handed over) for a target, "Q LP m mb ..." the same for a pattern, then "M t q verdict roots" followed by
// "root end steps" for every root: the verdict of the pair, and what each root ended with after how many steps.  No device is
// touched.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../moleculediffusiontransformer_amd/csrc/mdt_molsub.h"
#include "mol_host_graph.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  std::vector<Graph> targets, patterns;
  char tag[8];
  long pairs = 0, roots = 0, wrong = 0, steps_max = 0, undecided = 0;
  while (fscanf(f, "%7s", tag) == 1) {
    if (!strcmp(tag, "T") || !strcmp(tag, "Q")) {
      Graph g;
      if (!read_graph(f, g)) return 2;                            // exact sizes: a read past the counts is a report
      (tag[0] == 'T' ? targets : patterns).push_back(std::move(g));
    } else if (!strcmp(tag, "M")) {
      int t, q, verdict, count;
      if (fscanf(f, "%d %d %d %d", &t, &q, &verdict, &count) != 4) return 2;
      const Graph &a = targets[t], &p = patterns[q];
      int* code = new int[a.width];
      int* steps = new int[a.width];
      for (int r = 0; r < a.width; ++r) code[r] = -1, steps[r] = 0;
      const int got = mdt::sub_match_pair(a.atoms.get(), a.bonds.get(), a.n, a.nb, a.width, p.atoms.get(), p.bonds.get(), p.n, p.nb, p.width, code, steps);
      bool bad = got != verdict;
      int searched = 0;
      for (int r = 0; r < a.width; ++r) searched += code[r] >= 0;
      bad = bad || searched != count;
      for (int i = 0; i < count; ++i) {
        int root, end, made;
        if (fscanf(f, "%d %d %d", &root, &end, &made) != 3) return 2;
        bad = bad || root < 0 || root >= a.width || code[root] != end || steps[root] != made;
        steps_max = made > steps_max ? made : steps_max;
      }
      if (bad) {
        ++wrong;
        fprintf(stderr, "pair %d %d: verdict %d over %d roots, expected %d over %d\n", t, q, got, searched, verdict, count);
      }
      undecided += got == mdt::kSubCapped;
      roots += count;
      ++pairs;
      delete[] code;
      delete[] steps;
    } else {
      return 2;
    }
  }
  fclose(f);
  printf("%zu targets, %zu patterns, %ld pairs (%ld undecided), %ld roots, most steps of a root %ld, %ld wrong\n", targets.size(),
         patterns.size(), pairs, undecided, roots, steps_max, wrong);
  return wrong ? 1 : 0;
}
