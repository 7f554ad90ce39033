// Graph identity of generated molecules on gfx950: a SMILES string is one of many spellings of a molecule (OCC and CCO are ethanol
// twice), so "the same molecule" is decided on the molecular graph behind a row, not on the row.
//
//   k_mol_graph   compacted ids (R, L) + length (R) -> the graph of every row that passes mdt_smiles_check's rules: atom descriptors
//                 in order of appearance, bonds in order of creation, their counts; status and position as mdt_smiles_check
//   k_mol_key     the graph arrays -> one 64-bit key per row that does not depend on atom numbering, branch order, ring numbers
//                 or which end of a closure carries the bond symbol; 0 = no molecule
//   k_key_flags   per group: DUPLICATE where a lower candidate has the same non-zero key, KNOWN where the key is in a sorted set
//
// The definition (descriptor layout, bond orders, the rooted refinement hash and its limits) is written out at mdt_mol_graph and
// mdt_mol_key in include/mdt_hip.h; the scanner is k_smiles.hip's (mdt_smiles_scan.h), here with an emitter that records the graph.
//
// k_mol_graph: one lane per row, one 64-lane wave per workgroup, rows staged as class bytes in LDS exactly as in k_smiles.hip.
// Every lane owns `stride` bytes of LDS: [atoms 4L][bonds 4L][classes L][capacity L][position -> atom index L][branch stack L/2]
// [ring table 200], 4 * odd bytes, so equal offsets of the 32 lanes of an LDS lane group fall into 32 different banks.  The graph
// is built in LDS and written out by the whole wave, coalesced, zero beyond the counts; no array is indexed in registers.
//
// k_mol_key: one wave per row, LANE = ROOT.  All 64 lanes walk the same bond list for the same n rounds; control flow and every
// bond (a, b, order) are wave-uniform (scalar loads), only the labels differ.  Each lane keeps its own `lab` and `acc` columns in
// LDS as [atom][lane] 64-bit words (2 * L * 512 bytes): consecutive lanes read consecutive words, so a ds_read_b64 of the wave is
// two conflict-free halves, and no lane reads another lane's column, so there is no barrier.  n * |E| steps per row instead of
// n^2 * |E|; the sum over the roots is one butterfly reduction.  Lanes >= n contribute 0.  Rows without a molecule leave before
// any LDS work.
#include "mdt_kernels.h"
#include "mdt_device.h"
#include "mdt_smiles_scan.h"
#include "../../include/mdt_hip.h"

namespace mdt {

constexpr int kKeyFlagsMaxN = 1024;

// The per-lane bytes of LDS of k_mol_graph for rows of L positions: 4 * odd.
__host__ __device__ inline int molgraph_lane_stride(int L) {
  const int bytes = 4 * L + 4 * L + L + L + L + (L + 1) / 2 + 2 * kSmilesRings;
  const int words = (bytes + 3) / 4;
  return 4 * (words | 1);
}

__global__ __launch_bounds__(kSmilesLanes) void k_mol_graph(const int32_t* __restrict__ packed, const int32_t* __restrict__ length,
                                                            int R, int L, int stride, const uint8_t* __restrict__ classes,
                                                            const uint8_t* __restrict__ max_valence,
                                                            const uint32_t* __restrict__ elements, int32_t* __restrict__ natoms,
                                                            uint32_t* __restrict__ atoms, int32_t* __restrict__ nbonds,
                                                            uint32_t* __restrict__ bonds, uint8_t* __restrict__ status,
                                                            int32_t* __restrict__ position) {
  extern __shared__ uint32_t s_rows[];
  __shared__ uint8_t s_cls[256];
  __shared__ int s_na[kSmilesLanes], s_nb[kSmilesLanes];
  const int lane = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * kSmilesLanes;
  const int rows = (int)((int64_t)R - row0 < kSmilesLanes ? (int64_t)R - row0 : kSmilesLanes);
  for (int k = lane; k < 256; k += kSmilesLanes) s_cls[k] = classes[k];
  __syncthreads();
  uint8_t* base = (uint8_t*)s_rows;
  const int32_t* src = packed + row0 * L;
  const int total = rows * L;                                   // <= 64 * 64
  for (int i = lane; i < total; i += kSmilesLanes) {
    const int32_t id = src[i];
    const int r = i / L;
    base[r * stride + 8 * L + (i - r * L)] = (uint32_t)id < 256u ? s_cls[id] : (uint8_t)0;
  }
  __syncthreads();

  s_na[lane] = 0;
  s_nb[lane] = 0;
  if (lane < rows) {
    uint8_t* mine = base + lane * stride;
    MolGraphEmit emit;
    emit.atoms = (uint32_t*)mine;
    emit.bonds = (uint32_t*)(mine + 4 * L);
    const uint8_t* tok = mine + 8 * L;
    int8_t* cap = (int8_t*)(mine + 9 * L);                      // remaining capacity of the atom AT this position
    emit.index = mine + 10 * L;                                 // atom index (and the aromatic bit) of the atom AT this position
    uint8_t* stack = mine + 11 * L;                             // atom positions of the open branches' parents
    uint8_t* ring = stack + (L + 1) / 2;                        // 2 * number: opening atom, 2 * number + 1: its bond code
    uint64_t limits = 0;                                        // the ten maxima, one nibble each
    for (int k = 0; k < 10; ++k) limits |= (uint64_t)(max_valence[k] & 15u) << (4 * k);
    const int row_len = length[row0 + lane];
    const int n = row_len < 0 ? 0 : (row_len > L ? L : row_len);
    int over;
    const int viol = smiles_scan(tok, cap, stack, ring, L, n, limits, elements, over, emit);

    const int64_t row = row0 + lane;
    int na = 0, nb = 0;
    if (viol >= 0) {
      status[row] = MDT_SCREEN_MALFORMED;
      position[row] = viol;
    } else if (over != kNoPosition) {
      status[row] = MDT_SCREEN_OVERVALENT;
      position[row] = over;
    } else {
      status[row] = 0;
      position[row] = -1;
      na = emit.natoms;
      nb = emit.nbonds;
    }
    natoms[row] = na;
    nbonds[row] = nb;
    s_na[lane] = na;
    s_nb[lane] = nb;
  }
  __syncthreads();
  uint32_t* atoms_out = atoms + row0 * L;
  uint32_t* bonds_out = bonds + row0 * L;
  for (int i = lane; i < total; i += kSmilesLanes) {           // the whole rows, zero beyond the counts
    const int r = i / L, p = i - r * L;
    const uint32_t* lds = (const uint32_t*)(base + r * stride);
    atoms_out[i] = p < s_na[r] ? lds[p] : 0u;
    bonds_out[i] = p < s_nb[r] ? lds[L + p] : 0u;
  }
}

__global__ __launch_bounds__(64) void k_mol_key(const int32_t* __restrict__ natoms, const uint32_t* __restrict__ atoms,
                                                const int32_t* __restrict__ nbonds, const uint32_t* __restrict__ bonds, int L,
                                                uint64_t* __restrict__ key) {
  extern __shared__ uint64_t s_cols[];                          // lab [L][64], acc [L][64]
  const int64_t row = blockIdx.x;
  const int lane = threadIdx.x;
  const int n = natoms[row], nb = nbonds[row];
  const uint32_t* row_atoms = atoms + row * L;
  const uint32_t* row_bonds = bonds + row * L;
  // No molecule, counts no graph of this width can have, or a bond that names an atom the row does not have (it would index past
  // the columns): such a row has no key.
  if (!mol_graph_ok_wave(row_bonds, n, nb, L, lane)) {
    if (lane == 0) key[row] = 0;
    return;
  }
  uint64_t* lab = s_cols + lane;
  uint64_t* acc = s_cols + (size_t)L * 64 + lane;
  const uint64_t h = mol_root_hash(row_atoms, row_bonds, n, nb, lane, lab, acc, 64);
  uint64_t sum = lane < n ? mol_mix(h) : 0;
  for (int off = 32; off >= 1; off >>= 1) sum += shfl_xor_u64(sum, off);   // (a sum mod 2^64: exact in any order)
  if (lane == 0) key[row] = mol_key_final(sum, n, nb);
}

// One workgroup per group g; candidate c is row c * G + g.
__global__ __launch_bounds__(256) void k_key_flags(const uint64_t* __restrict__ key, int N, int G,
                                                   const uint64_t* __restrict__ known_key, int M, uint8_t* __restrict__ flags) {
  __shared__ uint64_t s_key[kKeyFlagsMaxN];
  const int g = blockIdx.x;
  for (int c = threadIdx.x; c < N; c += 256) s_key[c] = key[(int64_t)c * G + g];
  __syncthreads();
  for (int c = threadIdx.x; c < N; c += 256) {
    const uint64_t k = s_key[c];
    int f = 0;
    if (k != 0) {
      for (int o = 0; o < c; ++o)
        if (s_key[o] == k) {                                    // the first occurrence stands for all, whatever its status
          f |= MDT_SCREEN_DUPLICATE;
          break;
        }
      int lo = 0, hi = M;
      while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (known_key[mid] < k) lo = mid + 1; else hi = mid;
      }
      if (lo < M && known_key[lo] == k) f |= MDT_SCREEN_KNOWN;
    }
    flags[(int64_t)c * G + g] = (uint8_t)f;
  }
}

}  // namespace mdt

// ------------------------------------------------------------------------------------------------
// C ABI entry points of this translation unit (declared in include/mdt_hip.h)
// ------------------------------------------------------------------------------------------------
extern "C" int mdt_mol_graph(const int32_t* packed, const int32_t* length, int32_t L, int32_t R, const uint8_t* classes,
                             const uint8_t* max_valence, const uint32_t* elements, int32_t* natoms, uint32_t* atoms,
                             int32_t* nbonds, uint32_t* bonds, uint8_t* status, int32_t* position, void* stream) {
  if (R < 0) return mdt_bad("mdt_mol_graph: need R >= 0");
  if (L < 1 || L > mdt::kMolMaxL) return mdt_bad("mdt_mol_graph: need 1 <= L <= 64");
  if (R == 0) return 0;
  if (!packed || !length || !classes || !max_valence || !elements || !natoms || !atoms || !nbonds || !bonds || !status || !position)
    return mdt_bad("mdt_mol_graph: null pointer");
  const int stride = mdt::molgraph_lane_stride(L);
  const unsigned blocks = (unsigned)(((int64_t)R + mdt::kSmilesLanes - 1) / mdt::kSmilesLanes);
  hipLaunchKernelGGL(mdt::k_mol_graph, dim3(blocks), dim3(mdt::kSmilesLanes), (size_t)stride * mdt::kSmilesLanes,
                     (hipStream_t)stream, packed, length, R, L, stride, classes, max_valence, elements, natoms, atoms, nbonds, bonds,
                     status, position);
  return mdt_finish("mdt_mol_graph");
}

extern "C" int mdt_mol_key(const int32_t* natoms, const uint32_t* atoms, const int32_t* nbonds, const uint32_t* bonds, int32_t L,
                           int32_t R, uint64_t* key, void* stream) {
  if (R < 0) return mdt_bad("mdt_mol_key: need R >= 0");
  if (L < 1 || L > mdt::kMolMaxL) return mdt_bad("mdt_mol_key: need 1 <= L <= 64");
  if (R == 0) return 0;
  if (!natoms || !atoms || !nbonds || !bonds || !key) return mdt_bad("mdt_mol_key: null pointer");
  hipLaunchKernelGGL(mdt::k_mol_key, dim3((unsigned)R), dim3(64), (size_t)2 * L * 64 * sizeof(uint64_t), (hipStream_t)stream, natoms,
                     atoms, nbonds, bonds, L, key);
  return mdt_finish("mdt_mol_key");
}

extern "C" int mdt_key_flags(const uint64_t* key, int32_t N, int32_t G, const uint64_t* known_key, int32_t M, uint8_t* flags,
                             void* stream) {
  if (N < 1 || N > mdt::kKeyFlagsMaxN) return mdt_bad("mdt_key_flags: need 1 <= N <= 1024");
  if (G < 0 || M < 0) return mdt_bad("mdt_key_flags: need G >= 0 and M >= 0");
  if (G == 0) return 0;
  if (!key || !flags || (M > 0 && !known_key)) return mdt_bad("mdt_key_flags: null pointer");
  hipLaunchKernelGGL(mdt::k_key_flags, dim3((unsigned)G), dim3(256), 0, (hipStream_t)stream, key, N, G, known_key, M, flags);
  return mdt_finish("mdt_key_flags");
}
