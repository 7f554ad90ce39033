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
// The scan itself (smiles_scan) lives in mdt_smiles_scan.h, shared with k_molgraph.hip, which has it record the molecular graph;
// here it runs with the emitter that records nothing.
#include "mdt_kernels.h"
#include "mdt_device.h"
#include "mdt_smiles_scan.h"
#include "../../include/mdt_hip.h"

namespace mdt {

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
  SmilesNoEmit emit;                                           // the verdict alone: the graph goes to k_molgraph.hip
  const int viol = smiles_scan(tok, cap, stack, ring, L, n, limits, elements, over, emit);

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
extern "C" int mdt_smiles_check(const int32_t* packed, const int32_t* length, int32_t L, int32_t R, const uint8_t* classes,
                                const uint8_t* max_valence, const uint32_t* elements, uint8_t* status, int32_t* position,
                                void* stream) {
  if (R < 0) return mdt_bad("mdt_smiles_check: need R >= 0");
  if (L < 1 || L > mdt::kSmilesMaxL) return mdt_bad("mdt_smiles_check: need 1 <= L <= 128");
  if (R == 0) return 0;
  if (!packed || !length || !classes || !max_valence || !elements || !status || !position)
    return mdt_bad("mdt_smiles_check: null pointer");
  const int stride = mdt::smiles_lane_stride(L);
  const unsigned blocks = (unsigned)(((int64_t)R + mdt::kSmilesLanes - 1) / mdt::kSmilesLanes);
  hipLaunchKernelGGL(mdt::k_smiles_check, dim3(blocks), dim3(mdt::kSmilesLanes), (size_t)stride * mdt::kSmilesLanes,
                     (hipStream_t)stream, packed, length, R, L, stride, classes, max_valence, elements, status, position);
  return mdt_finish("mdt_smiles_check");
}
