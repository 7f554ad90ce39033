// The enumeration of csrc/mdt_molsub.h (sub_map_pair, sub_root_enumerate: the code k_sub_map runs) on the HOST, against rows written
// by tools/molmap_host_rows.py from the Python reference -- meant to be built with AddressSanitizer and UBSan, so that every array
// the functions touch has exactly the size the definition gives it:
//
//   python tools/molmap_host_rows.py rows.txt
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -I include \
//         tools/molmap_host_check.cpp -o molmap_host_check && ./molmap_host_check rows.txt
//
// Input, whitespace separated: "T L n nb atoms_present bonds_present" and the atom and bond words actually present (arrays of
// exactly that size are handed over) for a target, "Q LP m mb ..." the same for a pattern, then "M t q found capped embeddings
// cover", LP map bytes, "roots" and "root seen steps" for every root.  Every pair is also held against sub_match_pair: found != 0 is
// its match, found == 0 && capped != 0 its undecided.  No device is touched.
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
  long pairs = 0, roots = 0, wrong = 0, steps_max = 0, with_cap = 0, maps = 0;
  while (fscanf(f, "%7s", tag) == 1) {
    if (!strcmp(tag, "T") || !strcmp(tag, "Q")) {
      Graph g;
      if (!read_graph(f, g)) return 2;                            // exact sizes: a read past the counts is a report
      (tag[0] == 'T' ? targets : patterns).push_back(std::move(g));
    } else if (!strcmp(tag, "M")) {
      int t, q, count;
      unsigned long long want_found, want_capped, want_cover;
      unsigned want_emb;
      if (fscanf(f, "%d %d %llu %llu %u %llu", &t, &q, &want_found, &want_capped, &want_emb, &want_cover) != 6) return 2;
      const Graph &a = targets[t], &p = patterns[q];
      uint8_t* map = new uint8_t[p.width];                        // exactly LP bytes
      int* steps = new int[a.width];
      uint32_t* seen = new uint32_t[a.width];
      for (int r = 0; r < a.width; ++r) steps[r] = 0, seen[r] = 0;
      uint64_t found, capped, cover;
      uint32_t emb;
      mdt::sub_map_pair(a.atoms.get(), a.bonds.get(), a.n, a.nb, a.width, p.atoms.get(), p.bonds.get(), p.n, p.nb, p.width, &found, &capped, &emb, &cover, map,
                        steps, seen);
      bool bad = found != want_found || capped != want_capped || emb != want_emb || cover != want_cover;
      for (int i = 0; i < p.width; ++i) {
        int byte;
        if (fscanf(f, "%d", &byte) != 1) return 2;
        bad = bad || map[i] != byte;
      }
      if (fscanf(f, "%d", &count) != 1) return 2;
      for (int i = 0; i < count; ++i) {
        int root, its_seen, made;
        if (fscanf(f, "%d %d %d", &root, &its_seen, &made) != 3) return 2;
        bad = bad || root < 0 || root >= a.width || (int)seen[root] != its_seen || steps[root] != made;
        steps_max = made > steps_max ? made : steps_max;
      }
      const int old = mdt::sub_match_pair(a.atoms.get(), a.bonds.get(), a.n, a.nb, a.width, p.atoms.get(), p.bonds.get(), p.n, p.nb, p.width, nullptr, nullptr);
      bad = bad || (old == mdt::kSubFound) != (found != 0) || (old == mdt::kSubCapped) != (found == 0 && capped != 0);
      if (bad) {
        ++wrong;
        fprintf(stderr, "pair %d %d: found %llx capped %llx embeddings %u cover %llx, expected %llx %llx %u %llx\n", t, q,
                (unsigned long long)found, (unsigned long long)capped, emb, (unsigned long long)cover, want_found, want_capped, want_emb,
                want_cover);
      }
      with_cap += capped != 0;
      maps += emb;
      roots += count;
      ++pairs;
      delete[] map;
      delete[] steps;
      delete[] seen;
    } else {
      return 2;
    }
  }
  fclose(f);
  printf("%zu targets, %zu patterns, %ld pairs (%ld with a capped root), %ld roots, %ld embeddings, most steps of a root %ld, %ld wrong\n",
         targets.size(), patterns.size(), pairs, with_cap, roots, maps, steps_max, wrong);
  return wrong ? 1 : 0;
}
