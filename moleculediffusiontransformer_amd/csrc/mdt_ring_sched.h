// The loader schedule of the 32 KB ring of k_tf256.hip ("half a tile further ahead"), as plain C++: no HIP types, compiles for the
// host (tools/ring_sched_check.cpp replays descriptor streams against it) and for the device (the loader waves of k_tf256.hip).
//
// Ring: NSLOT = 4 slots of 32 KB, tile t lives in slot t % 4.  A tile is 32 pieces of 1 KB; loader wave iw issues piece q = 0..7
// to slot + q * 4096 + iw * 1024.  Barrier B(k) publishes tile k.  A compute wave consumes a weight tile in 4 units; it passes
// B(k) in front of unit 2 of tile k - 1 (phase(): fragment reads run two units ahead, so the reads of units 2 and 3 of tile k - 1
// may still be in flight there; those of units 0 and 1 have fed their MFMAs), or behind the whole tile where a sub-block ends.
//
// Read model.  Which unit reads a byte of a weight tile follows from the fragment addresses of phase() (frag_read, aP, aO):
//   split-bf16  P tile: row (fh, q, i) of 512 bytes = hi plane | lo plane of 256 bytes, 16-byte chunk c of a plane holds k-step
//                       (c ^ i) >> 2: unit = ((c ^ i) & 15) >> 2 -- units interleave every 64..128 bytes, NO piece is read by units
//                       0 and 1 only;
//               O tile: unit u reads [4096 u, 4096 u + 4096) of either 16 KB plane: unit = (offset & 16383) >> 12;
//   fp32        P tile: fragment (ft, st, lo) at ft * 8192 + st * 2048 + lo * 1024, unit = st:  unit = (offset & 8191) >> 11;
//               O tile: fragment (ct, sp, lo) at ct * 4096 + ..., unit u reads ct = 2 u, 2 u + 1:  unit = offset >> 13.
// The same for both feature halves and both row tiles (they differ in which lanes read, not in which bytes a unit reads).
// K / V tiles are read at once behind their barrier, scratch tiles are written and read by the compute waves: no units.
//
// Schedule.  A piece of a kind-P / kind-O tile t is EARLY when the tile that held the slot before it (t - 4) is a weight tile and
// the piece's 4 KB (all four loader waves' 1 KB) is read by units 0 and 1 of tile t - 4 only: dead at B(t - 3).  Behind B(k) the
// loader waves issue, in this order,
//     the late pieces of tile k + 2 (all of it when it has no early pieces)    into slot (k + 2) % 4, wholly free since B(k - 1),
//     the early pieces of tile k + 3                                           into the dead part of slot (k - 1) % 4,
//     their L2 touch of the stream, if it is this workgroup's turn (one load per wave).
// The one rule for everything else: a tile has early pieces only if t >= 4, its own kind is P or O and kind(t - 4) is P or O with a
// non-empty dead set -- K, V, scratch and vector tiles, every tile behind one of them in the same slot, and tiles 0..3 of a launch
// are issued whole at the old place (behind B(t - 2); tiles 0 and 1 in front of the loop).  Neighbours in the STREAM need no rule of
// their own: the allowance below counts what was really issued, and the last tiles of a launch are issued by turns that exist.
// For split-bf16 streams this makes P -> (slot of an O tile) and O -> (slot of an O tile) half-ahead and leaves every tile that
// follows a P tile in its slot whole; for fp32 streams every weight tile behind a weight tile is half-ahead.
//
// vmcnt allowance (per loader wave, operations return in issue order): B(k) needs every piece of tile k.  Its last piece is the
// last "late / whole" operation of turn k - 2, so what may stay in flight is the rest of turn k - 2 (early pieces + touch) and all
// of turn k - 1: Allowance below.  A wave with fewer operations than counted only waits longer.
//
// k_tf256.hip compiles this schedule with -DMDT_TUNING -DMDT_RING_HALF=1 only: measured, it is correct and slower than whole tiles
// (DESIGN.md 9).  The read model, the piece counts and the checker serve either schedule.
#pragma once

namespace mdt {
namespace ring {

enum : unsigned { T_P = 0, T_O = 1, T_K = 2, T_V = 3, T_SCRATCH = 4, T_SCRATCH_VEC = 5 };
constexpr int NSLOT = 4;            // ring slots
constexpr int SLOT_BYTES = 32768;   // one tile
constexpr int NPIECE = 8;           // pieces per loader wave and weight tile (q)
constexpr int NLOADER = 4;          // loader waves (iw)
constexpr int NUNIT = 4;            // units of a phase
constexpr unsigned WHOLE = 0xffu;   // piece mask of a whole weight tile

constexpr bool is_weight(unsigned kind) { return kind == T_P || kind == T_O; }

// destination of piece (iw, q) inside its slot
constexpr int piece_offset(int iw, int q) { return q * 4096 + iw * 1024; }

// the unit of phase() that reads byte `off` of a weight tile (every byte of a weight tile is read by exactly one unit)
constexpr int unit_of_byte(unsigned kind, bool f32, int off) {
  if (f32) return kind == T_P ? (off & 8191) >> 11 : off >> 13;
  if (kind == T_O) return (off & 16383) >> 12;
  return ((((off >> 4) & 15) ^ ((off >> 9) & 15)) & 15) >> 2;
}

// pieces q (bit q; all four waves' 1 KB) of a tile of this kind that units 0 and 1 read alone: dead once unit 1 is consumed
constexpr unsigned dead_pieces(unsigned kind, bool f32) {
  if (!is_weight(kind)) return 0u;
  unsigned m = 0u;
  for (int q = 0; q < NPIECE; ++q) {
    bool dead = true;
    for (int off = q * 4096; off < q * 4096 + 4096; off += 16)
      if (unit_of_byte(kind, f32, off) >= 2) dead = false;
    if (dead) m |= 1u << q;
  }
  return m;
}
constexpr unsigned DEAD_P_BF16 = dead_pieces(T_P, false), DEAD_O_BF16 = dead_pieces(T_O, false);
constexpr unsigned DEAD_P_F32 = dead_pieces(T_P, true), DEAD_O_F32 = dead_pieces(T_O, true);
static_assert(DEAD_P_BF16 == 0x00u && DEAD_O_BF16 == 0x33u, "split-bf16: only output tiles have a clean half");
static_assert(DEAD_P_F32 == 0x55u && DEAD_O_F32 == 0x0fu, "fp32 fragment tiles: both kinds have a clean half");

// early pieces of tile t (kind_t) whose slot held a tile of kind_prev (= tile t - 4) before it; 0 = the tile is issued whole
constexpr unsigned early_mask(bool f32, int t, unsigned kind_t, unsigned kind_prev) {
  if (t < NSLOT || !is_weight(kind_t) || !is_weight(kind_prev)) return 0u;
  return f32 ? (kind_prev == T_P ? DEAD_P_F32 : DEAD_O_F32) : (kind_prev == T_P ? DEAD_P_BF16 : DEAD_O_BF16);
}
constexpr unsigned late_mask(unsigned early) { return WHOLE & ~early; }
constexpr int popcount8(unsigned m) {
  int n = 0;
  for (int q = 0; q < NPIECE; ++q) n += (m >> q) & 1u;
  return n;
}

constexpr int NEARLY = NPIECE / 2;   // every non-empty early set is half a tile: the bytes per turn stay 32 KB in a steady stream
static_assert(popcount8(DEAD_O_BF16) == NEARLY && popcount8(DEAD_P_F32) == NEARLY && popcount8(DEAD_O_F32) == NEARLY, "half tiles");

// vector-memory operations loader wave iw issues for a whole tile of this kind (npw: pieces per wave of a K / V tile)
constexpr int pieces_of(unsigned kind, int iw, int npw, int vec_waves) {
  return kind == T_SCRATCH ? 0 : kind == T_SCRATCH_VEC ? (iw < vec_waves ? 1 : 0) : kind >= T_K ? npw : NPIECE;
}

// the counted wait of one loader wave: what may stay in flight in front of B(k)
struct Allowance {
  int prev_total = 0;   // operations of turn k - 1
  int prev_tail = 0;    // ... of them behind its late / whole part
  int prev2_tail = 0;   // operations of turn k - 2 behind its late / whole part
  constexpr int at_barrier() const { return prev_total + prev2_tail; }
  constexpr void turn(int late_or_whole, int early, int touch) {
    prev2_tail = prev_tail;
    prev_tail = early + touch;
    prev_total = late_or_whole + early + touch;
  }
};

}  // namespace ring
}  // namespace mdt
