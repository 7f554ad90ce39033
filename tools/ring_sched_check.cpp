// The loader schedule of csrc/mdt_ring_sched.h (what the loader waves of k_tf256.hip issue behind which barrier) replayed on the
// HOST over descriptor streams written by tools/ring_sched_dump.py -- host code only, meant to be built plainly and once more with
// AddressSanitizer and UBSan:
//
//   python tools/ring_sched_dump.py streams.txt
//   c++ -std=c++17 -O1 -g [-fsanitize=address,undefined] tools/ring_sched_check.cpp -o ring_sched_check && ./ring_sched_check streams.txt
//
// Input, whitespace separated, per stream: "S name f32 npw NT" and the NT descriptor words (kind | aux << 3) of ONE table.
// For every stream, with no L2 touch, a touch in every turn and a touch in every third turn, the program asserts
//   (0) the header's unit-of-a-byte model against the lane addresses of phase() written out here (aP / aO / frag_read offsets);
//   (a) no piece is issued into bytes a compute wave may still read or have in flight: a byte of weight tile t read by unit 0 / 1
//       is busy from B(t) to B(t + 1), by unit 2 / 3 to B(t + 2); a K / V / scratch slot from B(t - 1) to B(t + 2);
//   (b) every byte a unit reads (every piece of a K / V tile, the vector piece) was issued, and the counted wait in front of the
//       publishing barrier B(t) covers it: the piece is not among the last `allowance` operations of its wave (in issue order);
//   (c) every piece of every tile is issued exactly once.
// "--assume-p-dead" swaps in a WRONG rule (a split-bf16 P tile treated as if its pieces 0, 1, 4, 5 were dead): the program must
// then report violations of (a) -- the test runs it to see that the check bites.  No device is touched.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../moleculediffusiontransformer_amd/csrc/mdt_ring_sched.h"

using namespace mdt::ring;

static long g_bad = 0;
static void report(const std::string& s, const char* what, int t, int a, int b) {
  if (++g_bad <= 20) fprintf(stderr, "%s: %s (tile %d, %d, %d)\n", s.c_str(), what, t, a, b);
}

// (0) the bytes unit u reads, from the compute waves' addressing (k_tf256.hip: aP0 / aP / aO, frag_read): wave feature half fh,
// lane (i, g), read j = 2 q + lo
static bool check_model() {
  bool ok = true;
  for (int f32 = 0; f32 < 2; ++f32)
    for (unsigned kind = T_P; kind <= T_O; ++kind) {
      std::vector<int> seen(SLOT_BYTES / 16, -1);
      for (int u = 0; u < NUNIT; ++u)
        for (int fh = 0; fh < 2; ++fh)
          for (int lane = 0; lane < 64; ++lane)
            for (int j = 0; j < 4; ++j) {
              const int i = lane & 15, g = lane >> 4, q = j >> 1, lo = j & 1;
              int addr;
              if (f32) addr = kind == T_O ? lane * 16 + fh * 2048 + (2 * u + q) * 4096 + lo * 1024
                                          : lane * 16 + fh * 16384 + q * 8192 + u * 2048 + lo * 1024;
              else addr = kind == T_O ? i * 128 + ((4 * fh + g) ^ ((i >> 1) & 7)) * 16 + (2 * u + q) * 2048 + lo * 16384
                                      : ((fh * 16384 + i * 512 + ((g ^ i) & 15) * 16) ^ (64 * u)) + q * 8192 + lo * 256;
              if (addr < 0 || addr + 16 > SLOT_BYTES) { ok = false; continue; }
              if (seen[addr / 16] >= 0 && seen[addr / 16] != u) ok = false;      // two units read one chunk
              seen[addr / 16] = u;
              if (unit_of_byte(kind, f32 != 0, addr) != u || unit_of_byte(kind, f32 != 0, addr + 15) != u) ok = false;
            }
      for (int c : seen) ok = ok && c >= 0;                                      // the units read the whole tile
    }
  return ok;
}

struct Op { int tile, q; };   // q < 0: an L2 touch (no destination)

static void replay(const std::string& name, bool f32, int npw, const std::vector<unsigned>& d, int touch_every, bool wrong_rule) {
  const int NT = (int)d.size();
  const int VEC_WAVES = 3;
  auto kind = [&](int t) -> unsigned { return t >= 0 && t < NT ? (d[t] & 7u) : (unsigned)T_SCRATCH; };
  auto early = [&](int t) -> unsigned {
    if (wrong_rule && !f32 && t >= NSLOT && is_weight(kind(t)) && kind(t - NSLOT) == T_P) return DEAD_O_BF16;
    return early_mask(f32, t, kind(t), kind(t - NSLOT));
  };
  // busy_until(t, off): the barrier index at which byte `off` of tile t's slot is dead
  auto busy_until = [&](int t, int off) -> int {
    if (!is_weight(kind(t))) return t + 2;
    return unit_of_byte(kind(t), f32, off) < 2 ? t + 1 : t + 2;
  };
  for (int iw = 0; iw < NLOADER; ++iw) {
    std::vector<Op> fifo;                                    // this wave's operations in issue order
    std::vector<std::vector<int>> count(NT, std::vector<int>(NPIECE, 0)), index(NT, std::vector<int>(NPIECE, -1));
    auto issue = [&](int t, unsigned mask, int turn) {       // turn: the barrier the pieces are issued behind (-1: in front of the loop)
      const unsigned k = kind(t);
      const int n = pieces_of(k, iw, npw, VEC_WAVES);
      for (int q = 0; q < (is_weight(k) ? NPIECE : n); ++q) {
        if (is_weight(k) && !((mask >> q) & 1u)) continue;
        ++count[t][q];
        index[t][q] = (int)fifo.size();
        fifo.push_back(Op{t, q});
        if (k == T_SCRATCH_VEC) continue;                    // the vector area is double-buffered by the sub-block, not part of the ring
        const int prev = t - NSLOT;
        if (prev < 0) continue;
        const int lo = piece_offset(iw, q);
        for (int off = lo; off < lo + 1024; off += 16)       // (a)
          if (busy_until(prev, off) > turn) { report(name, "(a) piece issued into bytes still in use", t, q, turn); break; }
      }
      return is_weight(k) ? popcount8(mask) : n;
    };
    issue(0, WHOLE, -1);
    if (NT > 1) issue(1, WHOLE, -1);
    Allowance al;
    al.prev_total = NT > 1 ? pieces_of(kind(1), iw, npw, VEC_WAVES) : 0;
    unsigned em2 = 0u;
    for (int k = 0; k < NT; ++k) {
      const int allow = k + 1 < NT ? al.at_barrier() : 0;
      // (b): everything tile k needs from this wave is older than the last `allow` operations
      const unsigned kk = kind(k);
      const int need = is_weight(kk) ? NPIECE : pieces_of(kk, iw, npw, VEC_WAVES);
      for (int q = 0; q < need; ++q) {
        if (index[k][q] < 0) report(name, "(b) piece never issued before its barrier", k, q, iw);
        else if (index[k][q] >= (int)fifo.size() - allow) report(name, "(b) piece not covered by the counted wait", k, q, allow);
      }
      // behind B(k)
      const unsigned em3 = k + 3 < NT ? early(k + 3) : 0u;
      int n_late = 0, n_early = 0, touch = 0;
      if (k + 2 < NT) n_late = issue(k + 2, late_mask(em2), k);
      if (em3) n_early = issue(k + 3, em3, k);
      if (touch_every > 0 && k % touch_every == 0) { fifo.push_back(Op{-1, -1}); touch = 1; }
      al.turn(n_late, n_early, touch);
      em2 = em3;
    }
    for (int t = 0; t < NT; ++t) {                           // (c)
      const unsigned k = kind(t);
      const int need = is_weight(k) ? NPIECE : pieces_of(k, iw, npw, VEC_WAVES);
      for (int q = 0; q < NPIECE; ++q)
        if (count[t][q] != (q < need ? 1 : 0)) report(name, "(c) piece not issued exactly once", t, q, count[t][q]);
    }
  }
}

int main(int argc, char** argv) {
  bool wrong_rule = false;
  const char* path = nullptr;
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--assume-p-dead")) wrong_rule = true;
    else path = argv[i];
  }
  if (!path) return 2;
  if (!check_model()) {
    fprintf(stderr, "the unit-of-a-byte model of mdt_ring_sched.h does not match the fragment addresses\n");
    return 1;
  }
  FILE* f = fopen(path, "r");
  if (!f) return 2;
  char tag[8], name[128];
  long streams = 0, tiles = 0, halved = 0;
  while (fscanf(f, "%7s", tag) == 1) {
    int f32, npw, nt;
    if (strcmp(tag, "S") || fscanf(f, "%127s %d %d %d", name, &f32, &npw, &nt) != 4 || nt <= 0 || nt > (1 << 20) || npw < 0 || npw > NPIECE) return 2;
    std::vector<unsigned> d((size_t)nt);
    for (int i = 0; i < nt; ++i)
      if (fscanf(f, "%u", &d[i]) != 1 || (d[i] & 7u) > T_SCRATCH_VEC) return 2;
    for (int touch_every : {0, 1, 3}) replay(name, f32 != 0, npw, d, touch_every, wrong_rule);
    ++streams;
    tiles += nt;
    for (int t = NSLOT; t < nt; ++t) halved += early_mask(f32 != 0, t, d[t] & 7u, d[t - NSLOT] & 7u) != 0u;
  }
  fclose(f);
  printf("%ld streams, %ld tiles, %ld issued half a tile ahead, %ld violations\n", streams, tiles, halved, g_bad);
  return g_bad ? 1 : (streams ? 0 : 2);
}
