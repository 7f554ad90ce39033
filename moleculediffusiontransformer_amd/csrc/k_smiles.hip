// Well-formedness and valence of generated molecules on gfx950: what the reference's callers ask of every sample beside
// is_novel() -- `valid = Chem.MolFromSmiles(smi) != None` (draw_and_save, generative.py:954-994) -- as far as it can be decided in
// one pass over the string, on token ids, without leaving the device.
//
//   k_smiles_check     compacted ids (R, L) + length (R) -> status (0 | MALFORMED | OVERVALENT) and position per row
//
// The rule set is the one written out at mdt_smiles_check in include/mdt_hip.h (grammar, ring and branch bookkeeping, bond-order
// sums of unbracketed atoms).  It is NOT a SMILES parser in RDKit's sense: no aromaticity, no kekulisation, no hydrogens, no
// bracket-atom valence, no stereo consistency, and two bonds between the same pair of atoms pass.
//
// One lane per row, one 64-lane wave per workgroup.  A row's scan is a serial state machine, so the parallelism is across rows:
//   * the workgroup's 64 rows are read with coalesced loads (lane t reads word t, t + 64, ... of the 64 * L contiguous ids) and
//     stored into LDS as one CLASS BYTE per id (the 256-entry class table, itself staged in LDS), so the scan never touches the
//     row-major (R, L) image again -- read by one lane per row it would be a stride-L gather;
//   * every lane owns `stride` bytes of LDS: [classes L][remaining capacity per atom position L][branch stack L/2]
//     [ring table 100 x (atom, bond)].  The stride is 4 * odd bytes, so at equal offsets the 32 lanes of an LDS lane group sit
//     in 32 different banks whatever the access width;
//   * the scalar state (previous token kind, current atom, stack depth, pending bond, the 100 "ring is open" bits as two 64-bit
//     words, the lowest overvalent atom) lives in registers; no array is indexed in registers, so there is no scratch.
// A wave runs to its longest row and lanes on different token kinds take turns: accepted (tools/bench_smiles.py has the cost).
#include "mdt_kernels.h"
#include "mdt_device.h"
#include "../../include/mdt_hip.h"

namespace mdt {

// The class bytes (mdt_hip.h, mdt_smiles_check): 0 other | 1 + (c - 'A') | 27 + (c - 'a') | 53 + digit | then  - = # $ : / \ ( ) . [ ] % @ + *
constexpr int kClsUpper = 1, kClsLower = 27, kClsDigit = 53, kClsBond = 63, kClsOpen = 70, kClsClose = 71, kClsDot = 72,
              kClsLBracket = 73, kClsRBracket = 74, kClsPercent = 75, kClsAt = 76, kClsPlus = 77, kClsStar = 78;
constexpr int kClsMinus = kClsBond, kClsColon = kClsBond + 4;
enum { kPrevStart = 0, kPrevAtom, kPrevBond, kPrevDot, kPrevOpen, kPrevClose };
constexpr int kSmilesMaxL = 128, kSmilesRings = 100, kSmilesLanes = 64;
constexpr int kExempt = 127;                                   // capacity of an atom that is not judged (bracket, aromatic, '*')
constexpr int kNoPosition = 1 << 20;

__host__ __device__ __forceinline__ bool is_upper(int c) { return (unsigned)(c - kClsUpper) < 26u; }
__host__ __device__ __forceinline__ bool is_lower(int c) { return (unsigned)(c - kClsLower) < 26u; }
__host__ __device__ __forceinline__ bool is_digit(int c) { return (unsigned)(c - kClsDigit) < 10u; }
__host__ __device__ __forceinline__ bool is_bond(int c) { return (unsigned)(c - kClsBond) < 7u; }
// b c n o p s, as letters 0..25
__host__ __device__ __forceinline__ bool is_aromatic(int k) { return (unsigned)k < 26u && ((0x4E006u >> k) & 1u); }
// bond code 1..7 = - = # $ : / \ ; 0 = none, which bonds once
__host__ __device__ __forceinline__ int bond_order(int b) { return b >= 2 && b <= 4 ? b : 1; }
// The slot of an unbracketed uppercase atom in the max-valence table (B C N O P S F Cl Br I), -1: not an atom outside brackets.
__host__ __device__ __forceinline__ int organic_slot(int u) {
  switch (u) {
    case 'B' - 'A': return 0;
    case 'C' - 'A': return 1;
    case 'N' - 'A': return 2;
    case 'O' - 'A': return 3;
    case 'P' - 'A': return 4;
    case 'S' - 'A': return 5;
    case 'F' - 'A': return 6;
    case 'I' - 'A': return 9;
    default: return -1;
  }
}

// The per-lane bytes of LDS (see the top of the file) for rows of L positions: 4 * odd.
__host__ __device__ inline int smiles_lane_stride(int L) {
  const int bytes = L + L + (L + 1) / 2 + 2 * kSmilesRings;
  const int words = (bytes + 3) / 4;
  return 4 * (words | 1);
}

// The scan of one row (the rules: mdt_hip.h, mdt_smiles_check).  tok: its n <= L class bytes; cap (L), stack ((L + 1) / 2) and ring
// (2 * 100) are this row's work arrays, contents irrelevant before and after; limits: the ten maxima, one nibble each.
// -> the violation (>= 0: MALFORMED there) or -1, and `over`: the lowest overvalent atom or kNoPosition.  Host-callable, so
// that the rules can be run, and their array bounds checked, without a device.
__host__ __device__ inline int smiles_scan(const uint8_t* tok, int8_t* cap, uint8_t* stack, uint8_t* ring, int L, int n,
                                           uint64_t limits, const uint32_t* __restrict__ elements, int& over_out) {
  const int depth_max = (L + 1) / 2;
  int prev = kPrevStart, bond_prev = kPrevStart, cur = 0, depth = 0, pending = 0;
  uint64_t open_lo = 0, open_hi = 0;
  int over = kNoPosition, viol = -1;

  // order `o` more on atom `a`: the capacity goes down; below zero the atom is overvalent, and stays so
  auto bond_to = [&](int a, int o) {
    int v = cap[a];
    if (v == kExempt) return;
    v -= o;
    if (v < -100) v = -100;
    cap[a] = (int8_t)v;
    if (v < 0 && a < over) over = a;
  };

  int j = 0;
  while (j < n && viol < 0) {
    const int c = tok[j];
    int atom_cap = -1;                                          // >= 0: tokens [j, next) are an atom of this capacity
    int next = j + 1;
    if (is_upper(c)) {
      const int u = c - kClsUpper;
      int slot = organic_slot(u);
      if (j + 1 < n) {
        const int d = tok[j + 1];
        if (u == 'C' - 'A' && d == kClsLower + ('l' - 'a')) { slot = 7; next = j + 2; }
        if (u == 'B' - 'A' && d == kClsLower + ('r' - 'a')) { slot = 8; next = j + 2; }
      }
      if (slot < 0) viol = j;
      else atom_cap = (int)((limits >> (4 * slot)) & 15u);
    } else if (is_lower(c)) {
      if (is_aromatic(c - kClsLower)) atom_cap = kExempt;
      else viol = j;
    } else if (c == kClsStar) {
      atom_cap = kExempt;
    } else if (c == kClsLBracket) {
      int k = j + 1;
      while (k < n && is_digit(tok[k])) ++k;                    // isotope
      if (k >= n) viol = n;
      else {
        const int t = tok[k];
        if (is_upper(t)) {
          const uint32_t w = elements[t - kClsUpper];
          const int d = k + 1 < n ? tok[k + 1] : 0;
          if (is_lower(d) && ((w >> (d - kClsLower)) & 1u)) k += 2;
          else if ((w >> 26) & 1u) k += 1;
          else viol = k;
        } else if ((is_lower(t) && is_aromatic(t - kClsLower)) || t == kClsStar) {
          k += 1;
        } else {
          viol = k;
        }
      }
      if (viol < 0) {
        if (k < n && tok[k] == kClsAt) {                        // chiral
          ++k;
          if (k < n && tok[k] == kClsAt) ++k;
        }
        if (k < n && tok[k] == kClsUpper + ('H' - 'A')) {       // hcount
          ++k;
          if (k < n && is_digit(tok[k])) ++k;
        }
        if (k < n && (tok[k] == kClsPlus || tok[k] == kClsMinus)) {   // charge
          const int sign = tok[k];
          ++k;
          if (k < n && (tok[k] == sign || is_digit(tok[k]))) ++k;
        }
        if (k < n && tok[k] == kClsColon) {                     // class
          ++k;
          if (k >= n) viol = n;
          else if (!is_digit(tok[k])) viol = k;
          else
            while (k < n && is_digit(tok[k])) ++k;
        }
        if (viol < 0) {
          if (k >= n) viol = n;
          else if (tok[k] != kClsRBracket) viol = k;
          else { atom_cap = kExempt; next = k + 1; }
        }
      }
    } else if (is_bond(c)) {
      if (prev == kPrevAtom || prev == kPrevClose || prev == kPrevOpen) {
        bond_prev = prev;
        pending = c - kClsBond + 1;
        prev = kPrevBond;
      } else {
        viol = j;
      }
    } else if (is_digit(c) || c == kClsPercent) {
      const bool after_atom = prev == kPrevAtom || prev == kPrevClose;
      if (!(after_atom || (prev == kPrevBond && (bond_prev == kPrevAtom || bond_prev == kPrevClose)))) {
        viol = j;
      } else {
        int number = c - kClsDigit, last = j;
        if (c == kClsPercent) {
          if (j + 1 >= n) viol = n;
          else if (!is_digit(tok[j + 1])) viol = j + 1;
          else if (j + 2 >= n) viol = n;
          else if (!is_digit(tok[j + 2])) viol = j + 2;
          else {
            number = 10 * (tok[j + 1] - kClsDigit) + (tok[j + 2] - kClsDigit);
            last = j + 2;
          }
        }
        if (viol < 0) {                                         // 0 <= number <= 99
          const bool high = number >= 64;
          const uint64_t bit = (uint64_t)1 << (number & 63);
          if (!((high ? open_hi : open_lo) & bit)) {
            ring[2 * number] = (uint8_t)cur;
            ring[2 * number + 1] = (uint8_t)pending;
          } else {
            const int a = ring[2 * number], b = ring[2 * number + 1];
            if (a == cur || (b && pending && b != pending && !(b >= 6 && pending >= 6))) {
              viol = last;
            } else {
              const int o = bond_order(b ? b : pending);
              bond_to(a, o);
              bond_to(cur, o);
            }
          }
          if (high) open_hi ^= bit; else open_lo ^= bit;
          pending = 0;
          prev = kPrevAtom;
          next = last + 1;
        }
      }
    } else if (c == kClsOpen) {
      if ((prev == kPrevAtom || prev == kPrevClose) && depth < depth_max) {   // (depth < depth_max always: two tokens per level)
        stack[depth++] = (uint8_t)cur;
        prev = kPrevOpen;
      } else {
        viol = j;
      }
    } else if (c == kClsClose) {
      if ((prev == kPrevAtom || prev == kPrevClose) && depth > 0) {
        cur = stack[--depth];
        prev = kPrevClose;
      } else {
        viol = j;
      }
    } else if (c == kClsDot) {
      if ((prev == kPrevAtom || prev == kPrevClose) && depth == 0) prev = kPrevDot;
      else viol = j;
    } else {
      viol = j;
    }
    if (atom_cap >= 0) {                                        // a new atom at position j
      cap[j] = (int8_t)atom_cap;
      if (prev != kPrevStart && prev != kPrevDot) {
        const int o = bond_order(pending);
        bond_to(cur, o);
        bond_to(j, o);
      }
      pending = 0;
      cur = j;
      prev = kPrevAtom;
    }
    j = next;
  }
  if (viol < 0 && n > 0 && (!(prev == kPrevAtom || prev == kPrevClose) || depth > 0 || (open_lo | open_hi) != 0)) viol = n;

  over_out = over;
  return viol;
}

__global__ __launch_bounds__(kSmilesLanes) void k_smiles_check(const int32_t* __restrict__ packed, const int32_t* __restrict__ length,
                                                               int R, int L, int stride, const uint8_t* __restrict__ classes,
                                                               const uint8_t* __restrict__ max_valence,
                                                               const uint32_t* __restrict__ elements,
                                                               uint8_t* __restrict__ status, int32_t* __restrict__ position) {
  extern __shared__ uint32_t s_rows[];
  __shared__ uint8_t s_cls[256];
  const int lane = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * kSmilesLanes;
  const int rows = (int)((int64_t)R - row0 < kSmilesLanes ? (int64_t)R - row0 : kSmilesLanes);
  for (int k = lane; k < 256; k += kSmilesLanes) s_cls[k] = classes[k];
  __syncthreads();
  uint8_t* base = (uint8_t*)s_rows;
  const int32_t* src = packed + row0 * L;
  const int total = rows * L;                                   // <= 64 * 128
  for (int i = lane; i < total; i += kSmilesLanes) {
    const int32_t id = src[i];
    const int r = i / L;
    base[r * stride + (i - r * L)] = (uint32_t)id < 256u ? s_cls[id] : (uint8_t)0;
  }
  __syncthreads();
  if (lane >= rows) return;

  const uint8_t* tok = base + lane * stride;
  int8_t* cap = (int8_t*)(base + lane * stride + L);            // remaining capacity of the atom AT this position
  uint8_t* stack = base + lane * stride + 2 * L;                // atom positions of the open branches' parents
  uint8_t* ring = stack + (L + 1) / 2;                          // 2 * number: opening atom, 2 * number + 1: its bond code
  uint64_t limits = 0;                                          // the ten maxima, one nibble each
  for (int k = 0; k < 10; ++k) limits |= (uint64_t)(max_valence[k] & 15u) << (4 * k);
  const int row_len = length[row0 + lane];
  const int n = row_len < 0 ? 0 : (row_len > L ? L : row_len);
  int over;
  const int viol = smiles_scan(tok, cap, stack, ring, L, n, limits, elements, over);

  const int64_t row = row0 + lane;
  if (viol >= 0) {
    status[row] = MDT_SCREEN_MALFORMED;
    position[row] = viol;
  } else if (over != kNoPosition) {
    status[row] = MDT_SCREEN_OVERVALENT;
    position[row] = over;
  } else {
    status[row] = 0;
    position[row] = -1;
  }
}

}  // namespace mdt

// ------------------------------------------------------------------------------------------------
// C ABI entry point of this translation unit (declared in include/mdt_hip.h)
// ------------------------------------------------------------------------------------------------
extern "C" __attribute__((visibility("hidden"))) void mdt_set_error(const char* msg);  // mdt_api.cpp (not exported)

extern "C" int mdt_smiles_check(const int32_t* packed, const int32_t* length, int32_t L, int32_t R, const uint8_t* classes,
                                const uint8_t* max_valence, const uint32_t* elements, uint8_t* status, int32_t* position,
                                void* stream) {
  if (R < 0) {
    mdt_set_error("mdt_smiles_check: need R >= 0");
    return 2;
  }
  if (L < 1 || L > mdt::kSmilesMaxL) {
    mdt_set_error("mdt_smiles_check: need 1 <= L <= 128");
    return 2;
  }
  if (R == 0) return 0;
  if (!packed || !length || !classes || !max_valence || !elements || !status || !position) {
    mdt_set_error("mdt_smiles_check: null pointer");
    return 2;
  }
  const int stride = mdt::smiles_lane_stride(L);
  const unsigned blocks = (unsigned)(((int64_t)R + mdt::kSmilesLanes - 1) / mdt::kSmilesLanes);
  hipLaunchKernelGGL(mdt::k_smiles_check, dim3(blocks), dim3(mdt::kSmilesLanes), (size_t)stride * mdt::kSmilesLanes,
                     (hipStream_t)stream, packed, length, R, L, stride, classes, max_valence, elements, status, position);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    char buf[256];
    snprintf(buf, sizeof buf, "mdt_smiles_check: %s", hipGetErrorString(e));
    mdt_set_error(buf);
    return 1;
  }
  return 0;
}
