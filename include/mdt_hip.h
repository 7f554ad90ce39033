/*
 * mdt_hip.h -- C ABI of libmdt_hip.so, the MI355X (gfx950) kernels behind
 * QMDiffusion.sample / QMDiffusionForward.sample.
 *
 * The reference (lamm-mit/MoleculeDiffusionTransformer) is pure Python/PyTorch and has
 * no FFI of its own; the drop-in surface is the Python class pair QMDiffusion /
 * QMDiffusionForward (generative.py:718-914, :31-225).  This header is the native
 * boundary underneath that surface: plain device pointers, sizes and a hipStream_t
 * (passed as void*), no torch types.  Every entry point names the reference code
 * it replaces.  All pointers are DEVICE pointers to fp32 unless stated otherwise;
 * every call only enqueues work on `stream` (no allocation, no synchronisation), so
 * calls may be captured into a HIP graph.  Return value: 0 on success, non-zero on
 * error (message via mdt_last_error()).
 *
 * Layouts
 *   sampler state / noise / result : (B, C, L)   channel-major, as the reference
 *   U-Net activations              : (B, L, Cp)  token-major, Cp = C padded to 16
 *   context embedding              : (B, n, F)   as the reference
 */
#ifndef MDT_HIP_H
#define MDT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDT_ABI_VERSION 5

/* MDT_ABI_VERSION; a library built with -DMDT_TUNING (timing-only switches that may give WRONG results, csrc/mdt_kernels.h) sets
 * bit 30 on top -- the Python binding refuses such a library for sampling. */
int mdt_abi_version(void);
const char *mdt_last_error(void);
/* Process-wide tuning / test hooks (NOT part of the stable ABI; not needed for correct results): "pair_stride" = v > 0 places the two workgroups of
 * every pair-split MDT_OP_TF256 v workgroup ids apart whatever the op says (1: neighbours, i.e. different XCDs; 0: back to
 * the ops' own value); "tile16" = 0 | 1 | 2 forces a tile of the bf16 x bf16 GEMM (-1: automatic); "w16" = 0 | 1 turns that GEMM's all-bf16
 * epilogue (bf16 output, bf16 residual or none: 8 columns per lane, the residual requested under the main loop) off | on; "pair_capacity": see
 * mdt_pair_capacity.  Returns 0, or 1 for an unknown key. */
int mdt_set_tuning(const char *key, int32_t value);
/* Workgroups of a pair-split MDT_OP_TF256 launch that the current device keeps resident at the same time: compute units x
 * workgroups per compute unit (hipDeviceGetAttribute / hipOccupancyMaxActiveBlocksPerMultiprocessor; 256 on an MI355X), 0 if
 * unknown.  The two workgroups of a pair wait for each other inside the launch, so mdt_program_run never puts more than this
 * many into one launch: a larger batch runs as several launches over consecutive row-block ranges (same results).  The host
 * reads it to choose between the pair-split and the whole-workgroup form by batch size (generative.py::_wide).
 * mdt_set_tuning("pair_capacity", v > 0) replaces it (tests: force chunking on a small batch; 0 = back to the device's); the
 * override is a TEST HOOK: it is refused unless the process has MDT_TEST_HOOKS=1 in its environment. */
int32_t mdt_pair_capacity(void);
/* Which cross-attention core a MDT_OP_TF256 launch with T tokens per sample and Tk context rows runs (the launch's own
 * selection function, for tests): 1 = per-sample 4 x 4 MFMA blocks (T = 4), 0 = 16 x 16 tiles over the wave's 16 rows. */
int32_t mdt_tf256_block_core(int32_t T, int32_t Tk, int32_t cross);
/* Test hook: enqueue a kernel of n_workgroups workgroups that only HOLD compute units -- each allocates lds_bytes of LDS (<= 160
 * KiB: nothing else fits next to it) and spins for `ticks` of the 100 MHz real-time counter.  Used to break the co-residency
 * of pair-split launches on purpose (another stream holding most of the device) and check that the failure is reported.
 * NOT part of the stable ABI: refused unless the process has MDT_TEST_HOOKS=1 in its environment; at most 4096 workgroups and
 * 3 s (3e8 ticks). */
int mdt_test_occupy(int32_t n_workgroups, int32_t lds_bytes, uint64_t ticks, void *stream);

/* ------------------------------------------------------------------ */
/* U-Net evaluation as an op program                                   */
/* ------------------------------------------------------------------ */
/* The network (UNet1d.forward, modules.py:1144-1180) is lowered by the
 * Python host (moleculediffusiontransformer_amd/compiler.py) into a flat
 * list of fused ops over packed weights; mdt_program_run enqueues them.  */

enum mdt_space {
  MDT_SP_NONE = 0,
  MDT_SP_WEIGHT = 1, /* off = absolute float offset into the packed weight buffer            */
  MDT_SP_ACT = 2,    /* off = float offset PER SAMPLE; address = act + off * B               */
  MDT_SP_SHR = 3,    /* off = absolute float offset into the batch-invariant (shared) arena   */
  MDT_SP_EXT0 = 4    /* MDT_SP_EXT0 + i : off floats into bindings.ext[i]                      */
};
#define MDT_N_EXT 8

typedef struct mdt_ref {
  int32_t space;
  int32_t reserved;
  int64_t off;
} mdt_ref;

enum mdt_op_kind {
  MDT_OP_GEMM = 1,     /* nn.Linear / nn.Conv1d / nn.ConvTranspose1d phase as implicit GEMM with
                          fused norm-apply/FiLM/SiLU prologue and bias/GELU/residual epilogue
                          (modules.py:114-122, :135, :188, :317-319, :386-391, :486-516, :40-81) */
  MDT_OP_GN_STATS = 2, /* nn.GroupNorm statistics (modules.py:99-103, :485)                     */
  MDT_OP_ATTN = 3,     /* AttentionBase.forward core: softmax(q k^T * scale) v (modules.py:350-363) */
  MDT_OP_CONCAT = 4,   /* UpsampleBlock1d.add_skip: cat([x, skip * s], channel) (modules.py:828-829) */
  MDT_OP_PATCH = 5,    /* Patcher / Unpatcher rearrange (modules.py:230, :255)                   */
  MDT_OP_TIME_EMBED = 6, /* LearnedPositionalEmbedding.forward (modules.py:554-559)              */
  MDT_OP_GN_ACT = 8,   /* nn.GroupNorm + FiLM + SiLU applied in one pass: out = silu(gn(a) * (scale + 1) + shift)
                          (ConvBlock1d.forward before its convolution, modules.py:117-121); a -> out, p0 = gain,
                          p1 = bias, p3 = [scale | shift] or none (one row, or one per sample: mdt_op.film_bstride);
                          ints as MDT_OP_GN_STATS plus MDT_N_SILU                                                */
  MDT_OP_RCONV = 9,    /* row-stationary Conv1d (k = 1 | 3, C -> C channels, C in {128, 256}) with the ConvBlock1d prologue
                          computed in the kernel: out = bias + conv(silu(gn(s * a) * (scale + 1) + shift)) (+ res);
                          with a2 the input is cat([s * a, s2 * a2]) (2C channels, GroupNorm groups inside a half; the second
                          half's gain / bias / weight tiles follow the first's);
                          a, w = weight tiles, bias | none, out, res | none, p0 = gain, p1 = bias of the GroupNorm | none,
                          p3 = [scale | shift] | none (modules.py:117-121, :193-205)                             */
  MDT_OP_RESBLOCK = 10, /* a whole ResnetBlock1d with one GroupNorm group on a 64-token level (the U-Net's Patcher / Unpatcher,
                          modules.py:145-205, 208-257) in one launch, padded (cin, cout) = (16, 64) | (64, 16) | (16, 16), see MDT_K_CIN_REAL:
                          out = conv3(silu(gn(conv3(silu(gn(a))) + b1) (scale + 1) + shift)) + b2 + to_out(a);
                          a [B][64][cin], w = bf16 hi/lo MFMA fragments (conv1 | conv2 | to_out k-steps),
                          bias = gamma1 | beta1 | b1 | gamma2 | beta2 | (b2 + to_out bias), out [B][64][cout],
                          p3 = [scale | shift] | none                                                              */
  MDT_OP_TF128 = 11,   /* a whole Transformer1d (modules.py:469-524) of a 128-channel level in ONE launch: to_in (GroupNorm(32) +
                          Conv1d k=1), every TransformerBlock (self-attention, [cross-attention], feed-forward, :456-461) and
                          to_out (folded into the last feed-forward block); the residual stream never leaves the registers.
                          a = input [B][T][128], out = output, w = weight tile stream of all sub-blocks in consumption order
                          (projection tiles with their K columns permuted to the accumulator layout, see k_tf128.hip),
                          bias = every sub-block's vectors, p0 = tile descriptors (uint32 per tile: kind | aux << 2),
                          a2 = hoisted K|V rows of the FIRST cross-attention layer (layer l at + l * KV_LSTRIDE per-sample
                          floats), p1 = batch-invariant K|V rows for the second half of a dual batch; ints: enum mdt_tf128_i.
                          Optionally (MDT_F_RES_KIND) the level's ResnetBlock1d blocks (modules.py:145-205) run IN FRONT of the
                          transformer in the same launch (or alone, NBLOCKS = 0): res = the blocks' skip tensors (stored by kind 1,
                          read by kind 2), p3 = their FiLM rows                                                            */
  MDT_OP_TF256 = 12,   /* the same for a 256-channel level (32-row workgroups whose wave pairs split every chunk's features; the pair's
                          partial sums meet in scratch tiles of the ring).  Stream differences: 32 KB SUB-tiles (a [64][256]
                          projection tile = its two K halves, a [256][64] output tile = its two row halves), descriptors
                          kind (3 bits: 0 projection, 1 output, 2 K rows, 3 V rows, 4 scratch, 5 scratch + vectors of the next
                          sub-block) | aux << 3, two scratch descriptors after every sub-block; vectors: 768 floats per
                          sub-block ([bias 256] / [bq 512 | bo 256] / [b1 512 | b2 256]); NPOST = 8 sub-tiles; ints and
                          floats as MDT_OP_TF128 with C = 256.
                          MDT_F_NSPLIT = 2 (batches whose 32-row blocks do not fill the chip): every row block is served by a
                          PAIR of workgroups, half hh = 0 | 1 taking heads / hidden chunks / to_in output chunks / folded
                          to_out k chunks [hh n/2, (hh + 1) n/2); p0 then holds TWO descriptor tables of NT entries (half 0,
                          half 1; each sub-block's two scratch descriptors are followed by two more, kind 4, for the hand-off),
                          and the two workgroups hand each other their 32 x 256 partial sums inside the launch after every
                          sub-block: p3 = hand-off blocks, 2 * ceil(B T / 32) * 2 * 8192 floats; p2 = flag words (uint32):
                          64 diagnostic words (bit 0 of word 0 is raised if a poll timed out), then one 128-byte line per
                          (row block, half), counting hand-offs monotonically across launches -- zero them once, never between
                          launches.  The result does not depend on where the two workgroups run (k_tf256.hip)          */
  MDT_OP_PREP16 = 14,  /* A operand of a bf16 x bf16 GEMM: out (bf16 [B][R_IN][CIN], CIN / 2 floats per row) = bf16(prologue(a[.., A_COL +
                          c])); ints R_IN, LDA, CIN, A_COL, PRO, GROUPS, GSIZE, PRO_SILU and p0..p3 / eps as MDT_OP_GEMM;
                          WFMT = 2 (round 6): a is bf16 itself (LDA / A_COL in bf16 elements) -- LayerNorm (PRO 1) of the bf16
                          residual stream, statistics in fp32 on the exactly widened values; CIN <= 1024                     */
  MDT_OP_ATTN_CTX = 13, /* cross-attention core against the NORMALISED CONTEXT itself (K = V = c, shared by all heads and layers;
                          the per-layer key / value projections are folded into the query / output projections by the host):
                          a = q' [B][T * heads][128] (rows (token, head)), a2 = c [B | 1][Tk <= 64][LDKV], out [B][T * heads][128]
                          = softmax(q' c^T * scale) c; ints as MDT_OP_ATTN (LDQ / LDO unused)                              */
  MDT_OP_RES256 = 15,  /* a CHAIN of ResnetBlock1d blocks (modules.py:145-205) of a 256-channel level in ONE launch, 32-row workgroups that
                          keep their rows in registers from the first block to the last (csrc/k_res256.hip): kind 1: x = Block(x)
                          N_RES times, every block's output also stored as a skip tensor (DownsampleBlock1d / BottleneckBlock1d,
                          modules.py:680-721, :865-928); kind 2: x = Block(cat([x, s * skip[rb]])) (UpsampleBlock1d, :828-862).
                          a = x, out, res = skip tensors (addressed as MDT_OP_TF128's), w = weight sub-tile stream, bias = the blocks'
                          vectors, p0 = tile descriptors, p3 = the blocks' FiLM rows; ints: enum mdt_tf128_i with C = 256, the ResNet
                          fields, NT, NVEC = N_RES x (6 C | 9 C), and NPOST = taps of the block convolutions (3, or 1 when T = 1: only
                          the centre tap of a k = 3 convolution sees data); RES_PAIR1 / RES_PAIR2 are implied (GroupNorm groups of
                          64 channels on a 2C-channel input, 32 otherwise).  Stream: sub-tiles [64 features][128 k] in (tap, K half,
                          chunk) order per convolution; rows 0..31 of chunk c are output channels 32 c .., rows 32..63 channels
                          128 + 32 c ..; K columns in accumulator order (k-slot 32 st + 8 g + e = channel 16 (2 st + (e >> 2)) + 4 g +
                          (e & 3)).  Descriptors (HEADS of them, NT tiles in all) are SEGMENTS: kind (2 bits: 0 = a RUN of aux >= 1 consecutive sub-tiles
                          of the weight stream, which is stored in consumption order (aux = 0 is read as 1; the runs and single tiles sum to NT), 1 skip rows of block aux, 2 scratch, 3 scratch + the
                          vectors of block aux) | aux << 2; tile sequence: [3 (block 0)], then per block, kind 1: X nt X nt, kind 2: X nt X
                          8 S X 8 S X nt X nt (block1 on x, to_out on x, to_out on the skip, block1 on the skip, block2; X = 2, or 3 with aux = next block at a block's first X; nt = 8 taps; S = 1).  Vectors
                          per block: kind 1 [g1 | b1 | bias1 | g2 | b2 | bias2], kind 2 [g1 (2C) | b1 (2C) | bias1 | bias_to_out | g2 |
                          b2 | bias2].  WF32 as MDT_OP_TF256 (fp32 fragment sub-tiles).
                          NSPLIT = 2 (round 6; batches whose 32-row blocks do not fill the chip): a PAIR of workgroups per row block as
                          MDT_OP_TF256's pair split; a2 = the hand-off flags, p1 = the hand-off blocks (the SAME buffers as the
                          MDT_OP_TF256 ops of the level: shared flag lines, 32 KB blocks of which this op uses 16 KB), PAIR_STRIDE
                          as there, NFF = weight sub-tiles of ONE half.  Half hh streams output chunks 2 hh, 2 hh + 1 of every
                          convolution: sub-tiles in (tap, K half, chunk of the half) order, half 1's NFF sub-tiles behind half
                          0's; ONE descriptor table (the runs of both halves are equal, the tile sequence is the unsplit one with
                          half the weight runs); the pair's hand-offs use words 4..7 of the flag lines (one per compute wave; word 0
                          is MDT_OP_TF256's).  The result does not depend on where the two workgroups run.                     */
  MDT_OP_TBLOCK = 7    /* fused transformer sub-block, in place on x (TransformerBlock.forward, modules.py:456-461):
                          x += Attention(x) | x += Attention(x, context) | x += FeedForward(x); LayerNorm affine
                          folded into the projection weights, q/k/v/probabilities/hidden never leave registers */
};

/* prologue applied to the A operand of MDT_OP_GEMM while it is staged into LDS */
enum mdt_prologue {
  MDT_PRO_NONE = 0,
  MDT_PRO_LAYERNORM = 1, /* nn.LayerNorm over the K features of each row; p0 = gain, p1 = bias   */
  MDT_PRO_GROUPNORM = 2, /* normalise with stats from MDT_OP_GN_STATS (p2), p0 = gain, p1 = bias;
                            optional FiLM x*(scale+1)+shift (p3 = [scale(C) | shift(C)]); optional SiLU */
  MDT_PRO_SILU = 3       /* plain SiLU (MappingToScaleShift, modules.py:133-136)                 */
};

/* integer / float parameter slots of mdt_op, per kind */
/* common to the ring kernels' ops (MDT_OP_TBLOCK / RCONV / TF128 / TF256): size of the op's weight stream (w) in KB, 0 = unknown.
   The launch BEFORE such an op pulls that stream into the L2s while it finishes (its loader waves are idle by then). */
enum { MDT_W_KB = 23 };
enum mdt_gemm_i {
  MDT_G_R_OUT = 0,   /* M rows per sample of this GEMM                                           */
  MDT_G_R_IN = 1,    /* rows per sample of the A tensor                                           */
  MDT_G_LDA = 2,     /* floats per A row                                                          */
  MDT_G_CIN = 3,     /* channels consumed per tap (multiple of 16); K = taps * cin                */
  MDT_G_TAPS = 4,
  MDT_G_T_STRIDE = 5, /* source row of tap j for output row r: r*stride + j*dj + off; rows outside */
  MDT_G_T_DJ = 6,     /* [0, R_IN) read as zero AFTER the prologue (conv zero padding)             */
  MDT_G_T_OFF = 7,
  MDT_G_N = 8,       /* output features (multiple of 16)                                          */
  MDT_G_LDC = 9,     /* floats per output row                                                     */
  MDT_G_O_ROWS = 10, /* rows per sample of the output tensor                                      */
  MDT_G_O_STRIDE = 11, /* output row of GEMM row r: r*o_stride + o_off                             */
  MDT_G_O_OFF = 12,
  MDT_G_LDR = 13,    /* floats per residual row (residual uses the output row mapping)            */
  MDT_G_PRO = 14,    /* enum mdt_prologue                                                         */
  MDT_G_GROUPS = 15, /* GroupNorm groups                                                          */
  MDT_G_GSIZE = 16,  /* channels per group                                                        */
  MDT_G_PRO_SILU = 17, /* GROUPNORM prologue: apply SiLU after norm/FiLM                           */
  MDT_G_ACT = 18,    /* epilogue: 0 none, 1 exact-erf GELU                                         */
  MDT_G_M_MODE = 19, /* 0: M = B * R_OUT; 1: M = n_shared_rows * R_OUT; 2: M = R_OUT               */
  MDT_G_A_COL = 20,  /* first channel of the A row to consume                                     */
  MDT_G_O_COL = 21,  /* first column of the output row to write                                   */
  MDT_G_PHASES = 22, /* f > 1: ConvTranspose1d(k = 2f, stride f, padding f/2) as f output phases of 2 taps in ONE
                        launch (modules.py:74-81): phase ph uses weights [ph][N][K], T_OFF = (ph < f/2),
                        O_OFF = f * T_OFF + ph - f/2, O_STRIDE = f; 0 / 1: a plain GEMM                 */
  MDT_G_WFMT = 23    /* weight format: 0 = fp32 [N][K] (exact fp32 MFMA), or with a2 bound the hi (w) / lo (a2) bf16 planes of the
                        split product; 1 = ONE bf16 plane [N][K] in w: plain bf16 products (A rounded to bf16 after the prologue,
                        fp32 accumulation) -- the reduced-precision mode of the deep-UNet configuration;
                        2 = as 1 with the A operand ALREADY bf16 (written by MDT_OP_PREP16; LDA / A_COL in bf16 elements): both
                        operands stream through LDS-DMA; no prologue, stride, phases or output row mapping, cin % 64 == 0;
                        6 = as 2 and the OUTPUT is bf16 too (LDC / O_COL in bf16 elements): a tensor whose only reader is the next
                        bf16 x bf16 GEMM (feed-forward hidden layer); 10 = as 2 and ALSO a bf16 copy [rows][N] of the fp32 output
                        into p0 (the residual stream as the A operand of the next GEMM, written where it is produced);
                        38 (round 6) = as 6 and the RESIDUAL is bf16 too (LDR in bf16 elements; res may alias out): the bf16
                        residual stream of the plain-bf16 mode's transformer blocks -- one bf16 tensor is residual, output and the
                        next GEMM's A operand.
                        134 (round 6) = 6 with the LayerNorm of its A rows FOLDED into the GEMM: A is a raw bf16 row (the residual
                        stream), out = rstd (A W^T - mean colsum) + bias with the rows' mean / rstd over CIN gathered by the kernel
                        from the A fragments it multiplies, p0 = colsum [N] = sum_k W[n][k] of the bf16 weights (the host folds
                        the LayerNorm's gain into W and W bias_ln into bias), eps = f[0]; one tap, no residual, N / LDC / O_COL
                        multiples of 8.
                        Formats 2 / 6 / 10 end in a float4 epilogue: N, LDC, O_COL and LDR must be multiples of 4 and bias /
                        residual / out 16-byte aligned (bf16 out / copy: 8), otherwise the op is rejected;
                        16 = RING TILES (k_proj.hip, round 5): w holds N / 64 * CIN / 128 tiles of 32 KB, tile (chunk c, K half h)
                        at index c * (CIN / 128) + h = W[64 c .. 64 c + 64)[128 h .. 128 h + 128) as a bf16 hi plane [64][128]
                        followed by the lo plane (split-bf16 products); CIN in {128, 256}, N % 64 == 0, N <= 2048, prologue none or
                        LayerNorm (p0 / p1 both unbound = LayerNorm WITHOUT affine: the caller folded gain into the weights and
                        bias into the bias), one tap, bias / residual optional (the residual may alias out), no activation / row mapping;
                        17 = as 16 with fp32 FRAGMENT tiles (the layout of MDT_F_WF32) and exact fp32 MFMA products */
};
enum mdt_gemm_f { MDT_GF_EPS = 0 };

enum mdt_gn_i { MDT_N_ROWS = 0, MDT_N_LD = 1, MDT_N_GROUPS = 2, MDT_N_GSIZE = 3, MDT_N_SILU = 4,
                MDT_N_OUT16 = 5, /* MDT_OP_GN_ACT: 1 = out is bf16 [rows][ld] (A operand of a bf16 x bf16 GEMM) */
                MDT_N_CA = 6     /* MDT_OP_GN_ACT with a2 bound (round 6): the input is cat([a (CA channels, pitch CA), SCALE2 * a2 (LD - CA
                                    channels, pitch LD - CA)]) without the concatenated tensor; CA a multiple of GSIZE.  p2 (optional,
                                    with or without a2): also a raw bf16 copy [rows][LD] of that input */ };
enum mdt_gn_f { MDT_NF_EPS = 0, MDT_NF_SCALE2 = 1 };

enum mdt_rconv_i { MDT_R_T = 0, MDT_R_C = 1, MDT_R_LDA = 2, MDT_R_LDC = 3, MDT_R_LDR = 4, MDT_R_TAPS = 5,
                   MDT_R_GSIZE = 6 /* channels per GroupNorm group, 0 = no normalisation */, MDT_R_SILU = 7,
                   MDT_R_FILM_LD = 8 /* floats between the scale and the shift row */,
                   MDT_R_LDA2 = 9 /* floats per row of the second source (a2), if any */,
                   MDT_R_WF32 = 10 /* 1: w = fp32 fragment tiles, exact fp32 MFMA products (see MDT_F_WF32) */,
                   MDT_R_KSRC = 11 /* > 1 (round 5): a is [rows][KSRC * C] and its KSRC blocks of C channels accumulate into the C outputs,
                                      i.e. out = a W^T + bias (+ res) with K = KSRC * C == 1024 (tiles in the order source block /
                                      K half / feature chunk); one tap, no GroupNorm / FiLM / second source.  KSRC = 2 (C = 256): the two
                                      256-channel blocks of one tensor with 1 or 3 taps -- a strided Conv1d(k = 2 f + 1, stride f) in
                                      PATCH form: f consecutive tokens are one row of f * channels values and the convolution is k = 3
                                      over those rows */,
                   MDT_R_HALF_OUT = 12 /* 1 (C = 256, one source, no prologue): only output channels 0 .. 127 exist (LDC >= 128); the
                                      tile stream keeps the layout of all four 64-feature chunks, chunks 2 / 3 are never read */,
                   MDT_R_NB = 13 /* > 1 (one source, no prologue): NB * C output channels = NB convolutions of the same rows in one launch
                                      (tile streams, bias, residual and output columns of the blocks follow each other): a
                                      ConvTranspose1d(k = 2 f, stride f) in patch form writes f tokens x channels per input token */ };
enum mdt_rconv_f { MDT_RF_EPS = 0, MDT_RF_IN_SCALE = 1 /* factor on the rows of a -- with KSRC > 1 on EVERY K block of a */,
                   MDT_RF_IN_SCALE2 = 2 /* factor on the rows of a2 */ };
/* The KSRC > 1, HALF_OUT and NB > 1 forms move rows in 16-byte pieces: LDA, LDC and LDR (when res is bound) must be multiples of 4
   floats; HALF_OUT needs LDC (and LDR) >= 128, NB needs LDC (and LDR) >= NB * C.  mdt_program_create refuses anything else.      */
enum mdt_resblock_i { MDT_K_T = 0, MDT_K_CIN = 1, MDT_K_COUT = 2, MDT_K_FILM_LD = 3,
                      MDT_K_WF32 = 4 /* 1: w = fp32 MFMA fragments [step][row tile][half lo][64 lanes][4] (lane (i, g) float r =
                                        W[16 rt + i][the step's pair 8 g + 4 lo + r]), exact fp32 MFMA products */,
                      MDT_K_CIN_REAL = 5, MDT_K_COUT_REAL = 6 /* CIN / COUT are channel counts padded to 16; the GroupNorm
                                        statistics run over the first CIN_REAL / COUT_REAL channels (0 = all of them); padded
                                        gains, biases, weights -- hence outputs -- are zero */,
                      MDT_K_PATCH_IN = 7, MDT_K_PATCH_OUT = 8 /* p > 1 (round 5): the Patcher / Unpatcher rearrange folded into the
                                        block -- PATCH_IN: a is still patched, [T / p][CIN p] with a[l][c p + q] = x[l p + q][c];
                                        PATCH_OUT: out is written patched, [T / p][COUT p]; 0 / 1 = plain [T][C] */ };
enum mdt_resblock_f { MDT_KF_EPS = 0 };

enum mdt_attn_i {
  MDT_A_T = 0, MDT_A_TK = 1, MDT_A_HEADS = 2, MDT_A_LDQ = 3, MDT_A_LDKV = 4, MDT_A_LDO = 5,
  MDT_A_KV_BSTRIDE = 6, /* rows between consecutive samples' K/V (TK, or 0 for a batch-invariant context) */
  MDT_A_OUT16 = 7,      /* MDT_OP_ATTN: 1 = out is bf16 (LDO in bf16 elements), read by a bf16 x bf16 GEMM */
  MDT_A_QCOL = 8,       /* MDT_OP_ATTN: first float of q inside its rows (q | k | v projected by ONE GEMM into one tensor) */
  MDT_A_KCOL = 9,       /* ... and of k inside the a2 rows (v follows heads * 64 floats later)                          */
  MDT_A_SPLIT = 10,     /* MDT_OP_ATTN_CTX: 1 = the scores q' c^T as split-bf16 products (the default mode's arithmetic), 0 = exact fp32 */
  MDT_A_IN16 = 11       /* MDT_OP_ATTN: mask, 1 = q is bf16 (LDQ / QCOL in bf16 elements, multiples of 8), 2 = k | v are bf16 (LDKV / KCOL
                           likewise): the plain-bf16 mode's q | k | v GEMM writes bf16; widened exactly to fp32 in registers */
};
enum mdt_attn_f { MDT_AF_SCALE = 0 };

enum mdt_concat_i { MDT_C_ROWS = 0, MDT_C_CA = 1, MDT_C_CB = 2 };
enum mdt_concat_f { MDT_CF_SCALE_B = 0 };

enum mdt_patch_i { MDT_P_ROWS_IN = 0, MDT_P_C_IN = 1, MDT_P_LD_IN = 2, MDT_P_LD_OUT = 3, MDT_P_PATCH = 4,
                   MDT_P_INVERSE = 5 };

enum mdt_time_i { MDT_T_HALF = 0, MDT_T_LD = 1 };

/* MDT_OP_TBLOCK: a = x (in place), w = weight tile stream, bias = packed biases, a2 = hoisted K|V (cross) */
enum mdt_tblock_mode { MDT_TB_SELF = 0, MDT_TB_CROSS = 1, MDT_TB_FF = 2 };
enum mdt_tblock_i {
  MDT_B_MODE = 0, MDT_B_C = 1,      /* features (128 or 256)                                             */
  MDT_B_T = 2,                      /* tokens per sample (must divide 16)                                */
  MDT_B_NCHUNK = 3,                 /* heads (attention) or hidden/64 (feed-forward)                     */
  MDT_B_NBIAS = 4, MDT_B_TK = 5, MDT_B_KV_BSTRIDE = 6, MDT_B_LDKV = 7, MDT_B_HEADS = 8,
  MDT_B_KV2 = 11,                   /* cross blocks, 1: dual batch (both passes of classifier-free guidance in one launch,
                                       UNetCFG1d.forward, modules.py:1248-1253): the second half of the samples reads the
                                       batch-invariant K / V rows p1 (FixedEmbedding) instead of a2; the first half must be
                                       whole workgroups: (B / 2) % (64 / T) == 0 (C = 128), % (32 / T) (variants >= 2)  */
  MDT_B_POST = 10,                  /* feed-forward only, > 0: Transformer1d's closing Conv1d(k=1) folded in (modules.py:524):
                                       out = Wout (x + FF(x)) + bout; the W2 tiles hold Wout W2, POST = C/64 extra output
                                       tiles hold Wout (natural k order), the output bias holds Wout b2 + bout; x is left
                                       untouched                                                            */
  MDT_B_VARIANT = 9,                /* 0: 64-row workgroups, C = 128 (cross: <= 16 keys per 16 rows); 1: removed (round 3);
                                       2: 32-row workgroups, C = 256 (cross: <= 48 keys per 16 rows), weight
                                       stream packed as 128-wide sub-tiles (K halves / output-row halves);
                                       3: as 2, with the heads / hidden chunks of a row block split over two
                                       workgroups: out = scratch [2][B T][C] for their partial sums;
                                       4: chained form of 3 without the reduce launch: block input = a + res (res = the
                                       previous block's second partial | none), out = block output written by head group 0
                                       (never aliasing a), p2 = second head group's partial | none (one workgroup);  */
  MDT_B_WF32 = 12                   /* 1: w = fp32 FRAGMENT tiles (variant 0, round 5) / fp32 fragment SUB-tiles in the layout of MDT_OP_TF256
                                       (variants 2..4, round 6), exact fp32 MFMA products (see MDT_F_WF32)                      */
};
enum mdt_tblock_f { MDT_BF_EPS = 0, MDT_BF_SCALE = 1 };

/* MDT_OP_TF128 */
enum mdt_tf128_i {
  MDT_F_C = 0,           /* 128                                                                              */
  MDT_F_T = 1,           /* tokens per sample (divides 16)                                                    */
  MDT_F_NT = 2,          /* tiles in the stream (weight tiles + K / V tiles)                                  */
  MDT_F_NVEC = 3,        /* floats of vectors (multiple of 256, <= 8192): [to_in bias 128] then per block
                            [bq 64 heads | bo 128] (self), the same (cross), [b1 64 nff | b2 128] (feed-forward)  */
  MDT_F_TK = 4, MDT_F_KV_BSTRIDE = 5, MDT_F_LDKV = 6, MDT_F_HEADS = 7,
  MDT_F_HAS_IN = 8,      /* 1: starts with to_in (two projection tiles, GroupNorm gain / bias folded into them)  */
  MDT_F_NBLOCKS = 9 /* may be 0 (then HAS_IN = 0 too) when ResNet blocks are present */, MDT_F_NFF = 10 /* hidden / 64 */,
  MDT_F_NPOST = 11,      /* 2: to_out folded into the last feed-forward block (two extra output tiles), 0: none   */
  MDT_F_KV2 = 12,        /* 1: dual batch, as MDT_B_KV2 (first half = whole 64-row workgroups)                    */
  MDT_F_CROSS = 13,      /* 1: the blocks have a cross-attention sub-block                                        */
  MDT_F_KV_LSTRIDE = 14, /* per-sample floats between consecutive cross layers' K|V rows                         */
  /* MDT_OP_TF128 only: ResnetBlock1d blocks (modules.py:145-205) of the level IN FRONT of the transformer, same launch */
  MDT_F_RES_KIND = 15,   /* 0 none; 1: x = Block(x), N_RES times, every block's output ALSO stored as a skip tensor: block rb to
                            res + rb * (B * T * C floats) (the up path reads them back); 2: x = Block(cat([x, s * skip[rb]])) with
                            skip[rb] = res - rb * (B * T * C floats) (consumed in reverse order of production), s = f[SKIP_SCALE].
                            Stream per block, kind 1: 6 + 6 projection tiles (convolution taps x output halves, K columns in
                            accumulator order); kind 2: 2 to_out(x), [skip rows: descriptor 0 | (1 << 20 | rb) << 2], 2 to_out(skip),
                            6 block1(x), [skip rows], 6 block1(skip), 6 block2.  Vectors per block ahead of the transformer's: kind 1
                            [g1 | b1 | bias1 | g2 | b2 | bias2] (6 C), kind 2 [g1 (2C) | b1 (2C) | bias1 | bias_to_out | g2 | b2 | bias2]
                            (9 C).  p3 = the blocks' FiLM rows [scale C | shift C] each, contiguous (NFILM floats)             */
  MDT_F_N_RES = 16,
  MDT_F_RES_PAIR1 = 17,  /* GroupNorm groups of block1: 1 = 32 channels, 0 = 16 channels (block2: RES_PAIR2)                */
  MDT_F_RES_PAIR2 = 18,
  MDT_F_NFILM = 19,      /* FiLM floats staged behind the vectors (2 C per block, padded to a multiple of 256; NVEC + NFILM <= 8192) */
  /* MDT_OP_TF256 only */
  MDT_F_NSPLIT = 20,     /* 0 / 1: one workgroup per 32-row block; 2: a pair of workgroups per block (see MDT_OP_TF256)      */
  MDT_F_PAIR_STRIDE = 21,/* NSPLIT = 2: workgroup ids of a pair are this far apart (0 = 8: one XCD under the observed round-robin
                            placement; 1 = neighbours on different XCDs) -- speed only                                       */
  /* MDT_OP_TF128 and MDT_OP_TF256 */
  MDT_F_WF32 = 22        /* product type of every projection / convolution of the launch.  0: split-bf16 -- each 32 KB weight tile is a
                            bf16 hi plane then a lo plane, products hi*hi + hi*lo + lo*hi on bf16 MFMAs.  1: EXACT fp32 -- the same
                            tile holds the same weights as fp32 in MFMA-fragment order: for a tile of R x K weights (64 x 128
                            projection, 128 x 64 output) fragment (row tile rt, k-step st, half lo) is 1 KB at
                            ((rt * (K / 32) + st) * 2 + lo) * 1024 and float r of lane i + 16 g in it is
                            W[16 rt + i][k-slot 32 st + 8 g + 4 lo + r]; every product is a v_mfma_f32_16x16x4_f32 with fp32
                            accumulation, i.e. the reference's fp32 arithmetic (modules.py:314-320, :350-364, :386-391, :105-112) */
};
enum mdt_tf128_f { MDT_FF_EPS_LN = 0, MDT_FF_SCALE = 1, MDT_FF_EPS_GN = 2, MDT_FF_EPS_RES = 3, MDT_FF_SKIP_SCALE = 4 };

typedef struct mdt_op {
  int32_t kind;
  int32_t film_bstride; /* floats between the FiLM rows (p3) of consecutive samples: sample b reads p3 + b * film_bstride.  0 = ONE row
                           shared by the batch (sigma is a scalar: every sampling program).  Non-zero (a multiple of 4): one noise
                           level per sample (the "eval_rows" programs, KDiffusion_mod.forward); taken by MDT_OP_GN_ACT,
                           MDT_OP_RCONV (single source, GroupNorm prologue), MDT_OP_RESBLOCK and the GroupNorm prologue of MDT_OP_GEMM
                           (WFMT 0, M_MODE 0); refused on every other op (the chains of MDT_OP_TF128 / MDT_OP_RES256 stage one row).  Was `reserved` (always 0): an addition inside ABI version 5. */
  mdt_ref a;    /* GEMM A / GN input / ATTN q / CONCAT a / PATCH in / TIME c_noise values        */
  mdt_ref a2;   /* ATTN k (v = k + heads*64 floats) / CONCAT b / GEMM: bf16 lo plane of split weights:
                   when set, w is the bf16 hi plane [N][K] and the product is formed as hi*hi + hi*lo + lo*hi
                   on bf16 MFMAs with fp32 accumulation (needs cin % 32 == 0); unset = exact fp32 MFMA */
  mdt_ref w;    /* GEMM weights [N][K], K contiguous / TIME fourier weights                       */
  mdt_ref bias; /* GEMM bias [N]                                                                  */
  mdt_ref out;
  mdt_ref res;  /* GEMM residual                                                                  */
  mdt_ref p0, p1, p2, p3;
  int32_t i[24];
  float f[8];
} mdt_op;

typedef struct mdt_bindings {
  const float *weights;
  float *act; /* per-sample arena, act_floats_per_sample * B floats                               */
  float *shr; /* batch-invariant arena                                                            */
  float *ext[MDT_N_EXT];
} mdt_bindings;

typedef struct mdt_program mdt_program;

/* Validates and copies `n_ops` ops.  Returns NULL on error. */
mdt_program *mdt_program_create(const mdt_op *ops, int32_t n_ops);
void mdt_program_destroy(mdt_program *p);
int32_t mdt_program_num_ops(const mdt_program *p);
/* Enqueue ops [first, first+count) for batch size B (count < 0: to the end). */
int mdt_program_run(const mdt_program *p, const mdt_bindings *b, int32_t B, int32_t n_shared_rows,
                    int32_t first, int32_t count, void *stream);

/* ------------------------------------------------------------------ */
/* conditioning prelude                                                */
/* ------------------------------------------------------------------ */
/* generative.py:838-850 (QMDiffusion.sample) / :149-161 (QMDiffusionForward.sample):
 *   e[b,i,0:D1]      = gelu(fc1_w[d] * seq[b,i] + fc1_b[d])
 *   e[b,i,D1:D1+D2]  = PositionalEncoding1D: [sin(i*f_j) | cos(i*f_j)], f = inv_freq (D2/2 values)
 * (transformer.py:3456-3470).  out is (B, n, D1+D2). */
int mdt_cond_embed(const float *seq, const float *fc1_w, const float *fc1_b, const float *inv_freq,
                   float *out, int32_t B, int32_t n, int32_t D1, int32_t D2, void *stream);
/* The pos_emb_fourier_add form of the same prelude (generative.py:844-846, graphmodel.py:338-339): the positional
 * encoding is ADDED, e[b,i,d] = gelu(fc1_w[d] * seq[b,i] + fc1_b[d]) + PositionalEncoding1D(D2)[i,d] for d < D1 <= D2: the
 * reference's encoding returns its first `orig_ch` = D1 columns of [sin (D2/2 frequencies) | cos (D2/2)] (transformer.py:3456-3470),
 * so text_embed_dim may be smaller than embed_dim_position; out is (B, n, D1), inv_freq holds D2/2 frequencies. */
int mdt_cond_embed_add(const float *seq, const float *fc1_w, const float *fc1_b, const float *inv_freq,
                       float *out, int32_t B, int32_t n, int32_t D1, int32_t D2, void *stream);

/* ------------------------------------------------------------------ */
/* k-diffusion preconditioning + ADPM2 sampler update                   */
/* ------------------------------------------------------------------ */
/* KDiffusion_mod.denoise_fn input scaling (diffusion.py:810): xin[b,l,c] = c_in * x[b,c,l],
 * written token-major with channels padded to Cp (pad = 0). */
int mdt_precond_in(const float *x, float *xin, float c_in, int32_t B, int32_t C, int32_t L, int32_t Cp,
                   void *stream);
/* KDiffusion_mod.denoise_fn output (diffusion.py:811-814, clip :75-88):
 *   D = clip(c_skip * x + c_out * pred);   pred is token-major (B, L, Cp).
 * clip = clamp to [-1, 1] (dyn_scale == NULL: dynamic_threshold = 0.0, what every class of the reference passes), or dynamic
 * thresholding: dyn_scale[b] = max(quantile(|c_skip x + c_out pred|, q), 1) per sample (mdt_dyn_scale), D = clamp(., -s, s) / s.
 * The same optional argument on mdt_adpm2_mid / mdt_adpm2_next, whose denoise stage is this one.
 * The (L x Cp) tile of a sample is staged in LDS: L * (Cp + 1) * 4 <= 160 KiB (max_length = 1024 at Cp = 16: 68 KiB). */
int mdt_precond_out(const float *x, const float *pred, float *D, float c_skip, float c_out, int32_t B,
                    int32_t C, int32_t L, int32_t Cp, const float *dyn_scale, void *stream);
/* clip()'s dynamic threshold (diffusion.py:78-85): scale[b] = max(torch.quantile(|c_skip x[b] + c_out pred[b]|.flatten(), q), 1),
 * 0 < q <= 1, linear interpolation between the neighbouring order statistics as torch.quantile; C * L <= 32768. */
int mdt_dyn_scale(const float *x, const float *pred, float *scale, float c_skip, float c_out, float q, int32_t B,
                  int32_t C, int32_t L, int32_t Cp, void *stream);
/* ---- per-sample noise levels: KDiffusion_mod.forward (diffusion.py:820-844) and denoise_fn(sigmas=(B,)) (:798-814) as a batch.
 * sigma / c_in / c_skip / c_out / weight are DEVICE vectors of B floats (get_scale_weights / loss_weight, :789-796, :816-818, computed
 * by the host in the reference's fp32 tensor expressions).  Additions inside ABI version 5. ---- */
/* x_noisy = x0 + sigma[b] * noise (:828-829); xin = c_in[b] * x_noisy (:810), token-major, padded.  noise == NULL: the counter-based
 * generator of mdt_init_noise, keyed by (seed, step, sample0 + b): independent of how a batch is split. */
int mdt_noise_in_rows(const float *x0, const float *noise, const float *sigma, const float *c_in, float *x_noisy, float *xin,
                      uint64_t seed, uint32_t step, int64_t sample0, int32_t B, int32_t C, int32_t L, int32_t Cp, void *stream);
/* mdt_precond_in / mdt_precond_out / mdt_dyn_scale with one coefficient per sample. */
int mdt_precond_in_rows(const float *x, float *xin, const float *c_in, int32_t B, int32_t C, int32_t L, int32_t Cp, void *stream);
int mdt_precond_out_rows(const float *x, const float *pred, float *D, const float *c_skip, const float *c_out, int32_t B,
                         int32_t C, int32_t L, int32_t Cp, const float *dyn_scale, void *stream);
int mdt_dyn_scale_rows(const float *x, const float *pred, float *scale, const float *c_skip, const float *c_out, float q,
                       int32_t B, int32_t C, int32_t L, int32_t Cp, void *stream);
/* The objective's value in one pass (:838-844), the denoised tensor never written:
 *   loss[b] = weight[b] * mean_{c,l}((clip(c_skip[b] x_noisy + c_out[b] pred) - x0)^2),
 * clip as mdt_precond_out (dyn_scale NULL: clamp to [-1, 1]).  Fixed summation order: bitwise repeatable, and a sample's value does
 * not depend on its position in the batch.  C * L <= 32768. */
int mdt_loss_rows(const float *x0, const float *x_noisy, const float *pred, const float *c_skip, const float *c_out,
                  const float *weight, const float *dyn_scale, float *loss, int32_t B, int32_t C, int32_t L, int32_t Cp,
                  void *stream);
/* UNetCFG1d.forward guidance mix (modules.py:1253): out = um + (cond - um) * scale, token-major. */
int mdt_cfg_mix(const float *cond, const float *uncond, float *out, float scale, int64_t n, void *stream);
/* The mix with one scale per sample, rows of row_elems floats (a positive multiple of 4; any B, any total):
 *   out[b] = scale[b] == 1 ? cond[b] : uncond[b] + (cond[b] - uncond[b]) * scale[b]
 * in mdt_cfg_mix's evaluation order.  At scale 1 the reference skips guidance (modules.py:1248): the row is cond bit for bit and
 * uncond is not read.  out == cond (in place) is allowed.  scale: B floats on the device. */
int mdt_cfg_mix_rows(const float *cond, const float *uncond, float *out, const float *scale, int32_t B, int64_t row_elems,
                     void *stream);
/* First half of ADPM2Sampler.step (diffusion.py:506-508) fused with the denoise output:
 *   D = clamp(c_skip*x + c_out*pred, -1, 1); d = (x - D) / sigma; x_mid = x + d * dt_mid
 * and, for the next U-Net call, xin_mid = c_in_mid * x_mid (token-major, padded). */
int mdt_adpm2_mid(const float *x, const float *pred, float *x_mid, float *xin_mid, float c_skip,
                  float c_out, float sigma, float dt_mid, float c_in_mid, int32_t B, int32_t C, int32_t L,
                  int32_t Cp, const float *dyn_scale, void *stream);
/* Second half (diffusion.py:510-515):
 *   D = clamp(c_skip*x_mid + c_out*pred, -1, 1); d_mid = (x_mid - D) / sigma_mid;
 *   x = x + d_mid * dt_down;  x = x + noise * sigma_up   (in place on x)
 * and xin_next = c_in_next * x.  noise == NULL selects the counter-based generator:
 * Philox4x32-10 keyed by (seed, step), counter = global element index
 * (sample0 + b) * C * L + c * L + l, Box-Muller -- independent of how the batch is sharded.
 * tokens != NULL (only with xin_next == NULL, i.e. on the last update of a call): the decode step after the
 * path fused in, tokens[b,l] = argmax_c x[b,c,l] of the final x as int32 (generative.py:1212-1213, :1690-1691:
 * permute(0,2,1) -> argmax(dim=2); first maximum as torch.argmax). */
int mdt_adpm2_next(float *x, const float *x_mid, const float *pred, const float *noise, float *xin_next,
                   float c_skip, float c_out, float sigma_mid, float dt_down, float sigma_up,
                   float c_in_next, uint64_t seed, uint32_t step, int64_t sample0, int32_t B, int32_t C,
                   int32_t L, int32_t Cp, int32_t *tokens, const float *dyn_scale, void *stream);
/* One Euler move of ADPM2Sampler.step when the denoised tensor comes from a caller-supplied fn
 * (Sampler.forward(noise, fn, sigmas, num_steps) seam, diffusion.py:352, :502-515); all tensors (B, C, L):
 *   out = x_base + ((x_from - denoised) / sigma) * dt   [+ noise * sigma_up]
 * noise_mode 0: no noise term; 1: explicit `noise` tensor; 2: counter-based generator (seed, step, sample0). */
int mdt_adpm2_euler(const float *x_base, const float *x_from, const float *denoised, const float *noise,
                    float *out, float sigma, float dt, float sigma_up, int32_t noise_mode, uint64_t seed,
                    uint32_t step, int64_t sample0, int32_t B, int32_t C, int32_t L, void *stream);
/* The whole AEulerSampler.step after its one evaluation (diffusion.py:465-474), fused with the denoise output:
 *   D = clip(c_skip*x + c_out*pred); d = (x - D) / sigma; x = x + d * dt;  x = x + noise * sigma_up   (in place on x),
 *   dt = fp32(sigma_down - sigma),
 * and xin_next = c_in_next * x.  noise == NULL, tokens and dyn_scale as for mdt_adpm2_next.  An addition inside ABI version 5. */
int mdt_aeuler_next(float *x, const float *pred, const float *noise, float *xin_next, float c_skip, float c_out,
                    float sigma, float dt, float sigma_up, float c_in_next, uint64_t seed, uint32_t step,
                    int64_t sample0, int32_t B, int32_t C, int32_t L, int32_t Cp, int32_t *tokens,
                    const float *dyn_scale, void *stream);
/* KarrasSampler.step (diffusion.py:417-435) in three stages around its two evaluations; additions inside ABI version 5.
 * Churn (:424-425):   x_hat = x + noise_scale * (s_noise * noise),  noise_scale = fp32(sqrt(sigma_hat^2 - sigma^2)),
 *                     xin = c_in_hat * x_hat (token-major, padded).  x_hat may be x.  noise == NULL: counter-based generator. */
int mdt_karras_hat(const float *x, const float *noise, float *x_hat, float *xin, float noise_scale, float s_noise,
                   float c_in_hat, uint64_t seed, uint32_t step, int64_t sample0, int32_t B, int32_t C, int32_t L,
                   int32_t Cp, void *stream);
/* Euler move (:427-429): D = clip(c_skip*x_hat + c_out*pred); d = (x_hat - D) / sigma_hat; x_next = x_hat + dt * d,
 *                     dt = sigma_next - sigma_hat; d is kept for the correction; xin_next = c_in_next * x_next.
 * xin_next == NULL when sigma_next == 0 (no second evaluation: x_next is the step's result); tokens only then. */
int mdt_karras_mid(const float *x_hat, const float *pred, float *d, float *x_next, float *xin_next, float c_skip,
                   float c_out, float sigma_hat, float dt, float c_in_next, int32_t B, int32_t C, int32_t L,
                   int32_t Cp, int32_t *tokens, const float *dyn_scale, void *stream);
/* Correction (:432-434), the reference's line as it stands:
 *                     D = clip(c_skip*x_next + c_out*pred); d' = (x_next - D) / sigma_next; x = x_hat + half * (d + d'),
 *                     half = 0.5 * (sigma - sigma_hat) -- zero without churn, the step then returns x_hat.
 * x may be x_hat.  tokens != NULL: the fused decode of the final x. */
int mdt_karras_next(const float *x_hat, const float *x_next, const float *d, const float *pred, float *x,
                    float c_skip, float c_out, float sigma_next, float half, int32_t B, int32_t C, int32_t L,
                    int32_t Cp, int32_t *tokens, const float *dyn_scale, void *stream);
/* x = sigma0 * noise (diffusion.py:520); noise == NULL: counter-based generator as above. */
int mdt_init_noise(float *x, const float *noise, float sigma0, uint64_t seed, uint32_t step,
                   int64_t sample0, int32_t B, int32_t C, int32_t L, void *stream);
/* dst[0..n) = src[0..n) on the caller's stream (non-overlapping device buffers): selects the (scale | shift) rows of ONE evaluation out
 * of the table the time program fills for every evaluation of a call at once -- MappingToScaleShift of all 18 ResnetBlock1d blocks,
 * modules.py:125-142, evaluated per U-Net call in the reference (:1166-1170), once per sampling call here (rows are identical across the
 * batch: sigma is a scalar, diffusion.py:91-102).  Round 6, an addition inside ABI version 5. */
int mdt_copy_f32(float *dst, const float *src, int64_t n, void *stream);
/* DiffusionSampler final clamp (diffusion.py:590). */
int mdt_clamp(float *x, float lo, float hi, int64_t n, void *stream);
/* Inpainting merge (diffusion.py:539-542, :549): out = where(mask, src + sigma*noise, x);
 * mask is uint8 (B,C,L); noise may be NULL when sigma == 0. */
int mdt_inpaint_merge(float *x, const float *src, const uint8_t *mask, const float *noise, float sigma,
                      uint64_t seed, uint32_t step, int64_t sample0, int32_t B, int32_t C, int32_t L,
                      void *stream);
/* x += s * noise (inpaint re-noise, diffusion.py:546-547). */
int mdt_add_noise(float *x, const float *noise, float s, uint64_t seed, uint32_t step, int64_t sample0,
                  int32_t B, int32_t C, int32_t L, void *stream);
/* ---- fused inpainting entry and exit (ADPM2Sampler.inpaint, diffusion.py:526-549); additions inside ABI version 5.
 * The source is given either dense, src fp32 (B,C,L) (draft == NULL), or as draft token ids, draft int32 (B,L) (src == NULL), which
 * stand for their +-1 one-hot: src[b,c,l] = (c == draft[b,l]) ? 1 : -1 (encode_SMILES_into_one_hot, generative.py:1567-1569, :1603).
 * keep is uint8 (B,C,L), or with keep_per_token != 0 uint8 (B,L) broadcast over the channels (in_paint_mask before its
 * repeat 'b l -> b p l', generative.py:1600).  Non-zero = keep. ---- */
/* The entry of one resample in one pass (in place on x):
 *   x = keep ? src + sigma * n_src : x + renoise * n_re;   xin = c_in * x  (token-major, channels padded to Cp with 0)
 * -- mdt_add_noise(renoise, n_re) (skipped when renoise == 0: the first resample of a step), mdt_inpaint_merge(sigma, n_src),
 * mdt_precond_in(c_in), op for op: the result equals that composition bit for bit.  n_src / n_re == NULL: the counter-based
 * generator keyed by (seed, step_src / step_re) at the global element index (sample0 + b)*C*L + c*L + l, as those two. */
int mdt_inpaint_enter(float *x, float *xin, const float *src, const int32_t *draft, const uint8_t *keep,
                      int32_t keep_per_token, const float *n_src, const float *n_re, float sigma, float renoise,
                      float c_in, uint64_t seed, uint32_t step_src, uint32_t step_re, int64_t sample0, int32_t B,
                      int32_t C, int32_t L, int32_t Cp, void *stream);
/* The last merge (diffusion.py:549: sigma 0) and the decode (generative.py:1613-1614):
 *   x = keep ? src : x;   tokens[b,l] = argmax_c x[b,c,l]   (first maximum, as mdt_argmax_tokens; tokens may be NULL)
 * With draft ids and a per-token keep, a kept position's token is draft[b,l]. */
int mdt_inpaint_finish(float *x, const float *src, const int32_t *draft, const uint8_t *keep, int32_t keep_per_token,
                       int32_t *tokens, int32_t B, int32_t C, int32_t L, void *stream);
/* The entry of a refine call (noise a source up to the level of step i, the expression of diffusion.py:535, then :810), per
 * sample: a row with start[b] == step_i gets
 *   x = src + sigma * n;   xin = c_in * x  (token-major, channels padded to Cp with 0)
 * with separate multiply and add; a row with start[b] != step_i is written neither in x nor in xin.  start is int32 (B).
 * src / draft as mdt_inpaint_enter (exactly one of them); noise == NULL: the counter-based generator keyed by (seed, step) at the
 * global element index (sample0 + b)*C*L + c*L + l.  An addition inside ABI version 5. */
int mdt_refine_enter(float *x, float *xin, const int32_t *start, int32_t step_i, const float *src, const int32_t *draft,
                     const float *noise, float sigma, float c_in, uint64_t seed, uint32_t step, int64_t sample0, int32_t B,
                     int32_t C, int32_t L, int32_t Cp, void *stream);
/* The per-step entry of a refine call around a kept scaffold: launched in front of EVERY step i from min(start), it is the entry
 * of mdt_refine_enter and the merge of ADPM2Sampler.inpaint (diffusion.py:539-542, as a select) on one read of the state:
 *   start[b] >  step_i:  the row is written neither in x nor in xin;
 *   start[b] == step_i:  x = keep ? src + sigma * n_src : src + sigma * n_entry;
 *   start[b] <  step_i:  x = keep ? src + sigma * n_src : x;
 * with separate multiply and add, and for the rows that run xin = c_in * x (token-major, channels padded to Cp with 0).
 * src / draft as mdt_inpaint_enter (exactly one of them), keep / keep_per_token as mdt_inpaint_enter, start as mdt_refine_enter.
 * n_entry / n_src == NULL: the counter-based generator keyed by (seed, step_entry / step_src) at the global element index
 * (sample0 + b)*C*L + c*L + l.  An addition inside ABI version 5. */
int mdt_refine_keep_enter(float *x, float *xin, const int32_t *start, int32_t step_i, const float *src, const int32_t *draft,
                          const uint8_t *keep, int32_t keep_per_token, const float *n_entry, const float *n_src, float sigma,
                          float c_in, uint64_t seed, uint32_t step_entry, uint32_t step_src, int64_t sample0, int32_t B,
                          int32_t C, int32_t L, int32_t Cp, void *stream);
/* Decode step after the path (generative.py:1212-1213): tokens[b,l] = argmax_c x[b,c,l] (int32). */
int mdt_argmax_tokens(const float *x, int32_t *tokens, int32_t B, int32_t C, int32_t L, void *stream);

/* ------------------------------------------------------------------ */
/* candidate screening (csrc/k_screen.hip); additions inside ABI version 5 */
/* ------------------------------------------------------------------ */
/* What the reference's callers do with generated molecules (sample_loop_generative, generate_from_conditioning:
 * generative.py:1196-1291, :1685-1738): re-predict, compare with the target, ask is_novel (:1063) -- on token ids.  Row layout
 * everywhere: row r = c * G + g, candidate c of group g (a group is one target conditioning).  A molecule is its compacted id row:
 * the non-zero ids in order (the string of a character-level tokenizer, which skips id 0). */
/* Per row: the non-zero ids in order, left-packed and zero-padded, into packed (B,L); their number into length (B); into key (B)
 *   key = sum over j < length, mod 2^64, of mix((j << 32) | (uint32_t)packed[j]),
 *   mix(x): z = x + 0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB;
 *           z ^ (z >> 31)                                     (one splitmix64 step, 64-bit wrap-around arithmetic)
 * -- order-independent, so exact and deterministic; an empty row has key 0.  Equal rows have equal keys; the converse is never
 * assumed (mdt_screen_select confirms every key match on length and packed).  fwd_in fp32 (B,Lf), or NULL: the forward model's
 * input (generative.py:425-429 on ids), fwd_in[b,j] = (float)((double)packed[b,j] / x_norm) for j < min(length, Lf), 0 beyond.
 * packed must not be tokens. */
int mdt_tokens_compact(const int32_t *tokens, int32_t B, int32_t L, float *fwd_in, int32_t Lf, double x_norm, int32_t *packed,
                       int32_t *length, uint64_t *key, void *stream);
/* score[r] = (sum_i w_i * (p[r,i] - t[g,i])^2) / n in fp32: i ascending, separate subtract, square, multiply by w_i and add, one
 * divide by (float)n at the end; weights == NULL: w_i = 1.  p[r,i] = props[r * row_stride + i] (the forward sample (B,1,Lf) read
 * in place: row_stride = Lf); target is (G,n), weights (n), score (N*G).  1 <= n <= 64, row_stride >= n. */
int mdt_screen_score(const float *props, int64_t row_stride, const float *target, const float *weights, int32_t N, int32_t G,
                     int32_t n, float *score, void *stream);
/* status bits of a candidate (mdt_screen_select) */
enum mdt_screen_status {
  MDT_SCREEN_EMPTY = 1,     /* length == 0 */
  MDT_SCREEN_NONFINITE = 2, /* the score is a NaN or an infinity */
  MDT_SCREEN_DUPLICATE = 4, /* a candidate c' < c of the same group holds the same molecule (whatever the status of c') */
  MDT_SCREEN_KNOWN = 8,     /* the molecule is in the known set (mdt_screen_select_diverse: or closer to it than min_novelty) */
  MDT_SCREEN_CLOSE = 16,    /* mdt_screen_select_diverse only: closer than min_distance to a better candidate that was kept */
  MDT_SCREEN_MALFORMED = 32, /* mdt_smiles_check: the row breaks the grammar, or its ring / branch bookkeeping does not close */
  MDT_SCREEN_OVERVALENT = 64, /* mdt_smiles_check: well-formed, but an unbracketed atom's bond orders exceed its maximum; the
                                 screening call's kekulize: also a verdict != 0 of mdt_mol_hydrogens (no status bit is free) */
  MDT_SCREEN_SUBSTRUCTURE = 128 /* mdt_sub_match: a required pattern is missing or undecided, or a forbidden one present or undecided;
                                   the screening call's limits: also "a descriptor of mdt_mol_rings lies outside its bounds" (no
                                   status bit is free) */
};
/* Per group g: status uint8 (N*G) of every candidate; index int32 (G,K): the eligible (status == 0) candidates c in ascending
 * order of (score, c) -- ties go to the lower c -- and -1 in the slots beyond count[g] = min(K, number of eligible candidates).
 * score, key, packed (N*G,L), length as written by the two calls above.  The known set: known_key uint64 (M) ASCENDING,
 * known_packed int32 (M,L), known_len int32 (M), rows of the same width L, compacted and keyed as mdt_tokens_compact does; a
 * candidate is KNOWN when an entry of the run of known keys equal to its key has its length and its packed row.
 * Limits: 1 <= N <= 1024, 1 <= K <= N, 1 <= L <= 1024, M >= 0; the known pointers may be NULL only when M == 0. */
int mdt_screen_select(const float *score, const uint64_t *key, const int32_t *packed, const int32_t *length, int32_t L, int32_t N,
                      int32_t G, const uint64_t *known_key, const int32_t *known_packed, const int32_t *known_len, int32_t M,
                      int32_t K, uint8_t *status, int32_t *index, int32_t *count, void *stream);
/* mdt_screen_select with a per-row verdict from outside: reject uint8 (N*G), or NULL.  reject[r] is OR-ed into status[r] before
 * eligibility is decided, so a rejected candidate is never kept (mdt_smiles_check's status is the intended input; any non-zero
 * byte rejects).  DUPLICATE stays "a lower c holds the same molecule, whatever its status".  reject == NULL: mdt_screen_select. */
int mdt_screen_select_reject(const float *score, const uint64_t *key, const int32_t *packed, const int32_t *length, int32_t L,
                             int32_t N, int32_t G, const uint64_t *known_key, const int32_t *known_packed, const int32_t *known_len,
                             int32_t M, int32_t K, const uint8_t *reject, uint8_t *status, int32_t *index, int32_t *count,
                             void *stream);

/* ------------------------------------------------------------------ */
/* edit distance between molecules (csrc/k_edit.hip, csrc/k_screen.hip); additions inside ABI version 5 */
/* ------------------------------------------------------------------ */
/* The global Levenshtein distance (insert, delete, substitute: 1 each) between compacted rows a[0:la] and b[0:lb] as
 * mdt_tokens_compact writes them, of width 1 <= L <= 64 (one 64-bit word of Myers' / Hyyro's bit-vector recurrence per pair;
 * wider rows are out of scope).  Lengths are clamped to [0, L].  Ids are expected in [0, 64): an id outside that range matches
 * NOTHING, not even itself (the callers of the Python layer refuse such ids before any launch).  An empty row lies at the other
 * row's length.  R == 0: nothing is launched, 0 is returned. */
/* dist[r] (int32) = distance of row r of a to row r of b; a_packed, b_packed int32 (R,L), a_len, b_len int32 (R). */
int mdt_edit_distance_rows(const int32_t *a_packed, const int32_t *a_len, const int32_t *b_packed, const int32_t *b_len, int32_t L,
                           int32_t R, int32_t *dist, void *stream);
/* The known rows that one workgroup of mdt_edit_nearest walks; the known set is split into chunks of this many over the grid. */
#define MDT_EDIT_KNOWN_CHUNK 512
/* Per query row r of packed (R,L): dist[r] = the smallest distance to any of the M >= 1 known rows (known_packed int32 (M,L),
 * known_len int32 (M); any order, no keys), index[r] = the LOWEST known index that attains it.  The chunks' results are combined as
 * the minimum of (distance << 32) | index, one unsigned 64-bit word per query, which is the same in any order: the result does not
 * depend on how the work is split or scheduled.  best: workspace of R 64-bit words, allocated by the caller, contents irrelevant
 * before and after.  R <= 65535 * 64. */
int mdt_edit_nearest(const int32_t *packed, const int32_t *length, int32_t L, int32_t R, const int32_t *known_packed,
                     const int32_t *known_len, int32_t M, uint64_t *best, int32_t *dist, int32_t *index, void *stream);
/* mdt_screen_select with novelty and distinctness measured in edits; 1 <= L <= 64, the other limits as there.
 *  1. Bits 1, 2, 4 as mdt_screen_select.  Bit 8 (KNOWN): the known-set test of mdt_screen_select (when M > 0), or
 *     known_dist != NULL and known_dist[r] < min_novelty (known_dist int32 (N*G), e.g. mdt_edit_nearest's dist).
 *  2. The eligible (status == 0) candidates of a group in ascending order of (score, c).  In that order a candidate is KEPT when its
 *     distance to every candidate kept before it is >= min_distance, until K are kept: index[g,:] holds the kept candidates in the
 *     order they were kept, -1 after them, count[g] their number.
 *  3. Bit 16 (CLOSE) on every eligible candidate that was not kept and lies closer than min_distance to a kept candidate that
 *     precedes it in the order -- wherever the K-th was kept.  Kept rows stay 0; a row with one of bits 1..8 never gets bit 16.
 * min_distance <= 1 filters nothing (distinct rows lie 1 apart); with known_dist == NULL as well, the three outputs are
 * mdt_screen_select's bit for bit. */
int mdt_screen_select_diverse(const float *score, const uint64_t *key, const int32_t *packed, const int32_t *length, int32_t L,
                              int32_t N, int32_t G, const uint64_t *known_key, const int32_t *known_packed, const int32_t *known_len,
                              int32_t M, int32_t K, const int32_t *known_dist, int32_t min_novelty, int32_t min_distance,
                              uint8_t *status, int32_t *index, int32_t *count, void *stream);
/* mdt_screen_select_diverse with reject uint8 (N*G) or NULL, as mdt_screen_select_reject: the bits are OR-ed in at step 1, so a
 * rejected candidate is not eligible, is never kept and never pushes another out under min_distance (it gets no bit 16 either). */
int mdt_screen_select_diverse_reject(const float *score, const uint64_t *key, const int32_t *packed, const int32_t *length,
                                     int32_t L, int32_t N, int32_t G, const uint64_t *known_key, const int32_t *known_packed,
                                     const int32_t *known_len, int32_t M, int32_t K, const int32_t *known_dist, int32_t min_novelty,
                                     int32_t min_distance, const uint8_t *reject, uint8_t *status, int32_t *index, int32_t *count,
                                     void *stream);

/* ------------------------------------------------------------------ */
/* well-formedness and valence of token rows (csrc/k_smiles.hip); additions inside ABI version 5 */
/* ------------------------------------------------------------------ */
/* Is the row a molecule at all?  The reference's callers ask RDKit (valid = Chem.MolFromSmiles(smi) != None, generative.py:954-994);
 * this is a precisely defined single pass over the string instead: grammar, ring and branch bookkeeping, and the bond-order sums
 * of unbracketed atoms.  OK means "passes this check", not "RDKit parses it".
 *
 * packed int32 (R,L), length int32 (R) as mdt_tokens_compact writes them (length clamped to [0, L]); 1 <= L <= 128; R >= 0
 * (R == 0 launches nothing).  All pointers are device pointers.
 *   classes  uint8 (256): the class of id i, which stands for ONE character:
 *            0 other | 1 + (c - 'A') | 27 + (c - 'a') | 53 + digit | 63.. for  - = # $ : / \ ( ) . [ ] % @ + *  in this order.
 *            An id outside [0, 256) has class 0.  Class 0 is a violation wherever the scan meets it.
 *   max_valence uint8 (10): the maxima of B C N O P S F Cl Br I, in this order, each in [0, 15].
 *   elements uint32 (26): bit k (< 26) of word u: (uppercase u, lowercase k) is an element symbol; bit 26: uppercase u alone is.
 * status uint8 (R): 0, MDT_SCREEN_MALFORMED or MDT_SCREEN_OVERVALENT; position int32 (R): see below, -1 for an OK row.
 *
 * The rules.  n = length.  An empty row is OK.  The scan runs left to right and stops at the first token that violates a rule:
 * MALFORMED, position = that token's index.  Violations only visible at the end have position n.  OVERVALENT is judged only for
 * rows that are not malformed.  State: prev in {START, ATOM, BOND, DOT, OPEN, CLOSE}, the current atom, a stack of branch parents,
 * the pending bond symbol, a ring table for the numbers 0..99 (opening atom, bond symbol or none), a bond-order sum per atom.
 *  - Atoms outside brackets: B C N O P S F I, '*', aromatic b c n o p s; C directly followed by l is Cl, B by r is Br (two tokens,
 *    one atom, positioned at the first).  Any other letter, H included, is a violation at that letter.  An atom is allowed after
 *    every prev.  Unless prev is START or DOT it bonds to the current atom with the pending bond (order 1 if none); the order is
 *    added to both atoms' sums.  The new atom becomes current; the pending bond is cleared; prev = ATOM.
 *  - Bracket atoms: '[' isotope? symbol chiral? hcount? charge? class? ']'.  isotope: digits.  symbol: an uppercase letter -- with
 *    the next token if that is a lowercase letter and the pair is an element, else alone if it is one, else a violation at the
 *    uppercase letter -- or one of b c n o p s, or '*'; anything else is a violation at that token.  chiral: @ or @@.  hcount: H
 *    and at most one digit.  charge: + or -, optionally doubled or followed by one digit.  class: ':' and one or more digits (a
 *    non-digit after ':' is a violation at that token).  The first token that cannot continue the sequence and is not ']' is the
 *    violation; the end of the row inside a bracket gives position n.  One atom, positioned at '[', exempt from the valence check.
 *  - Bonds: - = # $ : / \ of orders 1 2 3 4 1 1 1, allowed when prev is ATOM, CLOSE or OPEN; prev = BOND.
 *  - Ring closures: a digit, or '%' and exactly two digits (a non-digit in either place is the violation; a missing digit gives
 *    position n).  Allowed when prev is ATOM or CLOSE, or BOND where that bond followed ATOM or CLOSE; otherwise the closure's
 *    first token is the violation.  After ')' the closure belongs to the branch's parent (lenient on purpose: CC(C)1CC1 is OK).
 *    A number that is not open is opened with (current atom, pending bond).  An open number is closed: a violation at the closure's
 *    last token when the opening atom is the current atom, or when both ends carry a bond symbol and the symbols differ ('/' and
 *    '\' are compatible with each other); else the order of whichever symbol is present (else 1) is added to both atoms and the number
 *    is free again.  In both cases the pending bond is cleared and prev = ATOM.
 *  - '(' is allowed when prev is ATOM or CLOSE: pushes the current atom, prev = OPEN.  ')' when prev is ATOM or CLOSE and the
 *    stack is not empty: pops into the current atom, prev = CLOSE.  '.' when prev is ATOM or CLOSE and the stack is empty:
 *    prev = DOT (rings may close across a dot).  Any other character is a violation at that token.
 *  - End of row: a non-empty row needs prev in {ATOM, CLOSE}, an empty stack and no open ring; otherwise MALFORMED at n.
 *  - Valence: an unbracketed, non-aromatic, non-'*' atom is overvalent when its sum exceeds its maximum; position = the atom
 *    position of the lowest-index overvalent atom.
 * Not checked: aromaticity and kekulisation, two bonds between the same pair of atoms, hydrogens, bracket-atom valence, stereo
 * consistency. */
int mdt_smiles_check(const int32_t *packed, const int32_t *length, int32_t L, int32_t R, const uint8_t *classes,
                     const uint8_t *max_valence, const uint32_t *elements, uint8_t *status, int32_t *position, void *stream);

/* ------------------------------------------------------------------ */
/* graph identity of token rows (csrc/k_molgraph.hip); additions inside ABI version 5 */
/* ------------------------------------------------------------------ */
/* Which molecule is the row?  A SMILES string is one of many spellings of a molecule (OCC and CCO are ethanol twice), so equality of
 * compacted rows is equality of spellings.  The reference's callers go through RDKit (Chem.MolFromSmiles, generative.py:954-994);
 * this is a precisely defined answer instead: the molecular graph the scan of mdt_smiles_check sees, and a 64-bit key of that graph
 * that does not depend on how the row spells it.
 *
 * The graph of a row (mdt_mol_graph).  packed, length, L, R, classes, max_valence, elements, status, position: as mdt_smiles_check,
 * the same scan, rules, classes and tables, the same status and position -- but 1 <= L <= 64: with at most 64 tokens there are at
 * most 64 atoms and at most 63 bonds (a ring bond costs two tokens); wider rows are refused before any launch.  For a row of
 * status 0 the scan also yields
 *  - atoms, in order of appearance: natoms int32 (R), atoms uint32 (R,L), one descriptor per atom:
 *      bits 0..4   the symbol's first letter, 0..25 for A..Z in either case; 26 for '*'
 *      bits 5..9   0, or 1 + (the symbol's second letter - 'a'): Cl and Br outside brackets, any two-letter element inside
 *      bit  10     aromatic: the symbol is one of b c n o p s in lower case (bracketed or not)
 *      bit  11     the atom is a bracket atom
 *      bits 12..16 formal charge + 9: '+' 1, '++' 2, '+d' d, '-' -1, '--' -2, '-d' -d; no charge, or unbracketed: 0
 *      bits 17..20 bracket H count: 'H' 1, 'Hd' d; absent, or unbracketed: 0
 *      bits 21..31 isotope number modulo 2048 (absent, or unbracketed: 0) -- the fields above take 21 bits, so 11 are left
 *    Chirality marks and the atom class are ignored.
 *  - bonds, in order of creation: nbonds int32 (R), bonds uint32 (R,L), a | b << 8 | order << 16 with a, b atom indices.  An atom
 *    that bonds to the current atom makes (current atom, new atom); a ring closure makes (opening atom, closing atom).  Orders:
 *    '-' '/' '\' 1, '=' 2, '#' 3, '$' 4, ':' 5, no symbol: 5 when both atoms are aromatic, else 1.  A ring closure takes
 *    whichever end's symbol is present.
 * Words beyond the counts are 0.  A row of status != 0, and an empty row, has natoms = nbonds = 0 and all-zero words.
 *
 * The key (mdt_mol_key).  mix = the splitmix64 step of mdt_tokens_compact.  n = natoms, E = the bonds, seed[a] = mix(atoms[a]),
 * ROOT = 0xA5A5A5A5A5A5A5A5, K = 0x100000001B3, all arithmetic mod 2^64.  For every root r in 0..n-1:
 *   1. lab = seed, then lab[r] = mix(seed[r] ^ ROOT).
 *   2. n rounds.  Each round: acc[a] = the sum, over the bonds at a to neighbour b (a bond listed twice counts twice), of
 *      mix(lab[b] + order * K); then lab[a] = mix(lab[a] ^ mix(acc[a])) for all a at once.
 *   3. H_r = the sum over a of mix(lab[a]).
 * key = mix(sum over r of mix(H_r) + n + (|E| << 32)); if that is 0, the key is 1.  KEY 0 MEANS "NO MOLECULE": natoms == 0, i.e. an
 * empty row or a row whose status is not 0 (and any row whose counts lie outside [0, L] or whose bonds name an atom >= natoms,
 * which mdt_mol_graph never writes).  Every combination over atoms, bonds and roots is a sum mod 2^64, so the key cannot depend on
 * atom numbering, branch order, ring numbers or which end of a closure carries the bond symbol.
 * Limits.  Equal graphs always give equal keys.  Unequal graphs can collide in principle: the key is a refinement hash, not a
 * canonical form (none was found among 2,100 random graphs of up to 20 atoms and the 684 graphs of up to 7 nodes and degree 4; the
 * rooting is what separates cubane from cuneane, decalin from bicyclopentyl, two cyclopropanes from cyclohexane).  It is not
 * RDKit's canonical SMILES: no hydrogen or bracket normalisation ([CH4] and C differ), no aromaticity perception (C1=CC=CC=C1 and
 * c1ccccc1 differ), and stereo is ignored (F/C=C/F equals F/C=C\F).  (mdt_mol_normalize writes graph arrays on which the first two
 * pairs have one key.)
 * mdt_mol_key takes the graph arrays (device pointers), so the graph is computed once.  R == 0 launches nothing. */
int mdt_mol_graph(const int32_t *packed, const int32_t *length, int32_t L, int32_t R, const uint8_t *classes,
                  const uint8_t *max_valence, const uint32_t *elements, int32_t *natoms, uint32_t *atoms, int32_t *nbonds,
                  uint32_t *bonds, uint8_t *status, int32_t *position, void *stream);
int mdt_mol_key(const int32_t *natoms, const uint32_t *atoms, const int32_t *nbonds, const uint32_t *bonds, int32_t L, int32_t R,
                uint64_t *key, void *stream);
/* flags uint8 (N*G), row r = c * G + g as in the selections: MDT_SCREEN_DUPLICATE when a candidate c' < c of the same group has the
 * same non-zero key, whatever the status of c' (the first occurrence stands for all); MDT_SCREEN_KNOWN when the key is non-zero and
 * is found, by binary search, in known_key: uint64 (M), ASCENDING as unsigned.  Key 0 gets neither bit.  1 <= N <= 1024, G >= 0
 * (G == 0 launches nothing), M >= 0; known_key may be NULL only when M == 0.  The flags are meant to be OR-ed into the `reject`
 * byte of the mdt_screen_select*_reject calls. */
int mdt_key_flags(const uint64_t *key, int32_t N, int32_t G, const uint64_t *known_key, int32_t M, uint8_t *flags, void *stream);

/* ------------------------------------------------------------------ */
/* Tanimoto similarity on graph fingerprints (csrc/k_molfp.hip, csrc/k_screen.hip); additions inside ABI version 5 */
/* ------------------------------------------------------------------ */
/* How similar are two molecules?  The edit distance above measures how two STRINGS are written (OCC lies two edits from CCO, the
 * same molecule); the reference's callers compare graphs (view_difference, generative.py:932-945: a maximum common substructure).
 * This is a precisely defined answer on the graph of mdt_mol_graph: a circular fingerprint of MDT_FP_BITS bits and the Tanimoto
 * similarity of two fingerprints.  Everything is integer arithmetic mod 2^64 and every result is exact.
 *
 * The fingerprint (mdt_mol_fp).  Inputs: the graph arrays natoms, atoms, nbonds, bonds of mdt_mol_graph (device pointers), rows of
 * width 1 <= L <= 64.  mix and K = 0x100000001B3 as in mdt_mol_key; there is no root.
 *  - Degree: deg[a] = the number of bond-list entries that name atom a, counted per END: a bond listed twice counts twice, and an
 *    entry (a, a), which mdt_mol_graph never writes, counts twice at a.
 *  - Round 0: id_0[a] = mix(atoms[a] | (uint64)deg[a] << 32).
 *  - Rounds r = 1..radius: acc[a] = the sum, over the bonds at a to neighbour b, of mix(id_{r-1}[b] + order * K) (an entry (a, a)
 *    adds its term twice); then id_r[a] = mix(id_{r-1}[a] ^ mix(acc[a])) for all atoms at once.
 *  - The fingerprint: MDT_FP_BITS = 1024 bits as 16 uint64 words.  For every atom a < natoms and every r in 0..radius bit
 *    id_r[a] & 1023 is set: word bit >> 6, bit bit & 63 of that word.  count = the number of set bits.  0 <= radius <= 3.
 *  - Rows without a molecule: natoms == 0 (an empty row, a row of status != 0) gives an all-zero fingerprint and count 0; so does a
 *    row whose counts lie outside [0, L] or whose bonds name an atom >= natoms (the rule of mdt_mol_key).
 * Tanimoto: inter = popcount(A & B), union = |A| + |B| - inter; the similarity is inter / union, and 0 when union == 0.  Fractions
 * are compared exactly, by cross-multiplication, never as floats.  A threshold crosses this interface as an integer sim_num in
 * [1, MDT_FP_SIM_DEN]: "at least as similar as the threshold" means union > 0 && inter * 65536 >= sim_num * union (32 bits suffice).
 * What this is NOT.  It is not RDKit's Morgan or ECFP fingerprint, and bits are not comparable with either.  The round-0 invariant
 * holds no implicit hydrogens (only what the descriptor holds).  Duplicate substructures are not removed (every atom sets a bit in
 * every round).  There is no aromaticity perception (C1=CC=CC=C1 and c1ccccc1 differ) and no stereo.  (On the arrays of
 * mdt_mol_normalize the two are one.)  Folding to 1024 bits can make
 * unequal environments share a bit, so unequal molecules can have similarity 1.  Equal graphs always give equal fingerprints: every
 * combination over the bonds is a sum mod 2^64 and the bit set does not depend on atom numbering.
 * fp uint64 (R,16), count int32 (R).  R == 0 launches nothing. */
#define MDT_FP_BITS 1024
#define MDT_FP_SIM_DEN 65536
int mdt_mol_fp(const int32_t *natoms, const uint32_t *atoms, const int32_t *nbonds, const uint32_t *bonds, int32_t L, int32_t R,
               int32_t radius, uint64_t *fp, int32_t *count, void *stream);
/* inter[r], uni[r] (int32) of row r of a_fp against row r of b_fp, both uint64 (R,16); the popcounts are taken from the words. */
int mdt_fp_tanimoto_rows(const uint64_t *a_fp, const uint64_t *b_fp, int32_t R, int32_t *inter, int32_t *uni, void *stream);
/* The known rows that one workgroup of mdt_fp_nearest walks; the known set is split into chunks of this many over the grid. */
#define MDT_FP_KNOWN_CHUNK 512
/* Per query row r of fp (R,16): index[r] = the LOWEST of the M >= 1 rows of known_fp uint64 (M,16) that attains the largest
 * similarity to it, inter[r] and uni[r] the counts of that pair (similarity 0 everywhere, e.g. an all-zero query: index 0).  The
 * chunks' results are combined as the maximum of (floor(inter * 2^31 / union) << 32) | (0xFFFFFFFF - index), one unsigned 64-bit
 * word per query: for unions up to 2048 distinct fractions differ by at least 2^-22, so the quotient orders them strictly and maps
 * equal fractions to equal values, and the result does not depend on how the work is split or scheduled.  best: workspace of R
 * 64-bit words, allocated by the caller, contents irrelevant before and after.  R <= 65535 * 64. */
int mdt_fp_nearest(const uint64_t *fp, int32_t R, const uint64_t *known_fp, int32_t M, uint64_t *best, int32_t *inter, int32_t *uni,
                   int32_t *index, void *stream);
/* mdt_screen_select_diverse_reject with similarity as a second way to be CLOSE: fp uint64 (N*G,16) and fp_count int32 (N*G) as
 * mdt_mol_fp writes them, 1 <= sim_num <= MDT_FP_SIM_DEN.  In step 2 a candidate is kept when, to every candidate kept before it,
 * its edit distance is >= min_distance (as there; min_distance <= 1 filters nothing) AND its similarity is not "at least
 * sim_num / 65536"; bit 16 goes to what either test passed over.  A row without a molecule has an all-zero fingerprint and is
 * similar to nothing.  fp == NULL and fp_count == NULL: mdt_screen_select_diverse_reject itself, the same launch, sim_num ignored. */
int mdt_screen_select_similar(const float *score, const uint64_t *key, const int32_t *packed, const int32_t *length, int32_t L,
                              int32_t N, int32_t G, const uint64_t *known_key, const int32_t *known_packed, const int32_t *known_len,
                              int32_t M, int32_t K, const int32_t *known_dist, int32_t min_novelty, int32_t min_distance,
                              const uint8_t *reject, const uint64_t *fp, const int32_t *fp_count, int32_t sim_num, uint8_t *status,
                              int32_t *index, int32_t *count, void *stream);

/* ------------------------------------------------------------------ */
/* Graph substructure match (csrc/k_molsub.hip, csrc/mdt_molsub.h); additions inside ABI version 5 */
/* ------------------------------------------------------------------ */
/* Does the molecule contain this fragment?  OCC contains CO; a string search says no.  This is a precisely defined answer on the
 * graph of mdt_mol_graph.  It is not RDKit's HasSubstructMatch and not SMARTS: patterns are written in the same SMILES dialect and
 * parsed by the same scan.
 *
 * Inputs.  Target rows: natoms, atoms, nbonds, bonds of mdt_mol_graph, R rows of width 1 <= L <= 64.  Pattern rows: the same four
 * arrays for 1 <= P <= MDT_SUB_MAX_PATTERNS patterns of width 1 <= LP <= MDT_SUB_MAX_WIDTH.  n and m are the atom counts of target
 * and pattern.
 * Atom rule.  Pattern atom p accepts target atom t when ((p ^ t) & mask(p)) == 0, mask(p) = (bracket(p) ? 0xFFFFF000 : 0) |
 * (first letter of p == 26 ? 0 : 0x7FF): symbol and aromatic bit must be equal unless the pattern atom is '*'; a bracketed pattern
 * atom also wants equal charge, H-count and isotope fields (an unbracketed target atom has all three 0, so [N] accepts N); the bracket
 * bit itself never counts.
 * Bond rule.  A pattern bond (a, b, order) is satisfied under a map f when the target's bond list holds an entry between f(a) and
 * f(b), in either direction, with the same order (the orders of mdt_mol_graph: cc is 5, CC is 1).  A pattern entry listed twice asks
 * the same thing twice.
 * Match.  Pattern q occurs in a row when an injective f: pattern atoms -> target atoms satisfies both rules: subgraph monomorphism,
 * not the induced kind (extra target bonds between mapped atoms are fine).  A disconnected pattern ('.') needs all its parts on
 * distinct atoms.
 * The search is part of the definition, because its cap is.  Pattern atoms are taken in index order (order of appearance; the scan
 * guarantees that every atom after the first of a component has a bond to an earlier atom).  Back-bonds of p: the pattern entries
 * with max(a, b) == p, other end min(a, b) (the scan can write a > b, as in C(C1)1).  Candidates of p under a partial map, taken in
 * ascending target index: compat[p] & ~used & AND over the back-bonds (e, o) of p of adj_o[f(e)], where compat[p] is the 64-bit set
 * of target atoms that p accepts and adj_o[u] the set of atoms joined to u by an entry of order o.
 * Decided before any search: a pattern or target with no molecule gives no match -- natoms == 0, counts outside [0, width], or a
 * bond naming an atom >= natoms (the rule of mdt_mol_key); m > n gives no match; some compat[p] == 0 gives no match; m == 1 matches
 * iff compat[0] != 0.  Otherwise every root r in compat[0] runs a depth-first search with f(0) = r.  One STEP is one assignment
 * f(p) = t for p >= 1; the search succeeds when atom m - 1 is assigned; a root about to make step number MDT_SUB_MAX_STEPS + 1 is
 * abandoned (capped).  Per (row, pattern): MATCH if any root succeeds, UNDECIDED if none succeeds and at least one was capped, NO
 * MATCH otherwise.  The result does not depend on scheduling: a root may stop early once another has succeeded, and for no other
 * reason.  The cap is a definition, not a measurement: *.*.*.*.*.*.*.* against 64 atoms is 64^8 maps, and a kernel without a cap
 * would be a hang.
 * What no scan writes: a target entry of an order outside 1..5 joins nothing; a pattern with such an entry gives no match; a
 * pattern entry (p, p) is part of what p accepts -- only a target atom with an entry (t, t) of that order is in compat[p].
 * What this is and is NOT.  A decided answer (match or no match) does not depend on how target or pattern is spelled; which rows
 * come out undecided can depend on the spelling.  There are no implicit hydrogens, so [CH4] does not accept C; no aromaticity
 * perception, so c1ccccc1 is not found in C1=CC=CC=C1; no stereo, no recursive or logical atom expressions, and no mapping is
 * returned.  The fingerprint of mdt_mol_fp is no pre-filter for this: the atom's degree enters its round 0, so a fragment's bits
 * are not a subset of its host's bits.
 * Outputs: bit q of match[r] / undecided[r] (uint32 (R)) is the verdict for pattern q; the two words never share a bit.  flags uint8
 * (R) or NULL: MDT_SCREEN_SUBSTRUCTURE when (match[r] & need) != need or ((match[r] | undecided[r]) & ban) != 0, else 0 --
 * conservative both ways: an undecided required pattern counts as missing, an undecided forbidden one as present.  need and ban
 * may only have bits below P and may not overlap.  R == 0 launches nothing. */
#define MDT_SUB_MAX_PATTERNS 32
#define MDT_SUB_MAX_WIDTH 32
#define MDT_SUB_MAX_STEPS 4096
int mdt_sub_match(const int32_t *natoms, const uint32_t *atoms, const int32_t *nbonds, const uint32_t *bonds, int32_t L, int32_t R,
                  const int32_t *p_natoms, const uint32_t *p_atoms, const int32_t *p_nbonds, const uint32_t *p_bonds,
                  int32_t LP, int32_t P, uint32_t need, uint32_t ban,
                  uint32_t *match, uint32_t *undecided, uint8_t *flags, void *stream);

/* Which atoms match, and how often?  (mdt_sub_match returns no mapping; this call does.  An addition inside ABI version 5.)
 * Everything up to the search is mdt_sub_match's, word for word: the inputs, the atom rule, the bond rule, the back-bonds, the
 * candidates in ascending target index, and what is decided before any search.  It is as little SMARTS or RDKit's
 * GetSubstructMatches as that call is, with the same limits (no implicit hydrogens, no aromaticity perception, no stereo).
 * The enumeration.  Every root r in compat[0] runs the depth-first search of mdt_sub_match with f(0) = r to the END of its tree:
 * when atom m - 1 is assigned the full map f is an EMBEDDING, it is counted, and the walk goes on at the same depth with the
 * candidates above the one just taken.  Steps are counted as there, one per assignment f(p) = t, p >= 1, and the root is abandoned
 * (capped) when step MDT_SUB_MAX_STEPS + 1 would be made.  A root ends with the number of embeddings it saw, and capped or not.  Up
 * to its first success the walk and the step count are mdt_sub_match's, so "saw at least one embedding" is that call's success of
 * the root and "capped and saw none" its abandoned root: bit q of match[r] is found[r][q] != 0, bit q of undecided[r] is
 * found[r][q] == 0 && capped[r][q] != 0.  No root stops for another, so every root's end is defined whatever the scheduling.
 * Outputs per (row r, pattern q), every word written, all zero for a pair decided "no match" before the search:
 *  found uint64 (R,P)       bit t: root t saw an embedding -- the set of target atoms that can play pattern atom 0.
 *  capped uint64 (R,P)      bit t: root t was abandoned.  A root can have both bits.
 *  embeddings uint32 (R,P)  the maps seen over all roots; exact when capped == 0.
 *  cover uint64 (R,P)       every target atom that lies in some embedding seen; exact when capped == 0.
 *  map uint8 (R,P,LP)       1 + f(p) for the FIRST map of the LOWEST found root, 0 elsewhere and beyond m.  When no root below that
 *                           one is capped it is the lexicographically smallest of all embeddings.
 * A pattern of one atom: found = cover = compat[0], embeddings = popcount, map[0] = 1 + the lowest accepted atom.
 * The count is of ANCHORS, not atom sets: popcount(found), the target atoms that can play pattern atom 0.  C(F)(F)F counts CF3
 * carbons (6 embeddings each, one anchor); [N+](=O)[O-] counts nitro nitrogens; CC counts every carbon with a carbon neighbour, not
 * the C-C bonds.  Write the fragment with its distinctive atom first.
 * flags uint8 (R) or NULL, from count_lo / count_hi uint8 (P), both NULL or both given (flags needs them): with c =
 * popcount(found) and u = popcount(capped & ~found), the flag is MDT_SCREEN_SUBSTRUCTURE unless for every q count_lo[q] <= c and
 * c + u <= count_hi[q] -- conservative both ways: an abandoned root that saw nothing may be an anchor (it counts against the upper
 * bound) or none (it does not count towards the lower).  c + u <= 64, so a count_hi of 64 or more is no upper bound.
 * The refusals before any launch are mdt_sub_match's, and the two about count_lo / count_hi / flags.  R == 0 launches nothing.  The
 * worst case is 64 roots of MDT_SUB_MAX_STEPS steps per pair, and once more for one of them (the first map is found by running the
 * lowest found root's walk again, csrc/k_molsub.hip). */
int mdt_sub_map(const int32_t *natoms, const uint32_t *atoms, const int32_t *nbonds, const uint32_t *bonds, int32_t L, int32_t R,
                const int32_t *p_natoms, const uint32_t *p_atoms, const int32_t *p_nbonds, const uint32_t *p_bonds,
                int32_t LP, int32_t P, const uint8_t *count_lo, const uint8_t *count_hi,
                uint64_t *found, uint64_t *capped, uint32_t *embeddings, uint64_t *cover, uint8_t *map, uint8_t *flags,
                void *stream);

/* ------------------------------------------------------------------ */
/* Implicit hydrogens and a Kekule check (csrc/k_molh.hip, csrc/mdt_molh.h); additions inside ABI version 5 */
/* ------------------------------------------------------------------ */
/* How many hydrogens does each atom carry, and is the row, where it is written with lower-case atoms, a molecule at all?
 * mdt_smiles_check exempts aromatic atoms from every valence rule, so c1cccc1 passes it; the reference's callers would see RDKit
 * refuse it (Chem.MolFromSmiles(smi) is None, generative.py:954-994).  This is a precisely defined answer on the graph of
 * mdt_mol_graph: per atom its hydrogens and whether it still needs a double bond, per row whether those double bonds can be placed
 * (a Kekule structure exists), and the molecular formula.  It is not RDKit's sanitisation.
 *
 * Inputs.  natoms, atoms, nbonds, bonds of mdt_mol_graph (device pointers), R rows of width 1 <= L <= 64; 1 <= max_steps <=
 * MDT_MOLH_MAX_STEPS.  A row that is no molecule -- natoms == 0, counts outside [0, L], a bond naming an atom >= natoms (the rule of
 * mdt_mol_key) -- has verdict 0, atom -1 and all-zero outputs.
 * Per atom.  sum1(a) = the sum over the bond entries at a of the order, an entry of order 5 counted as 1; an entry listed twice
 * counts twice; an entry (a, a), which mdt_mol_graph never writes, counts twice at a and is never an edge below.  Normal valences:
 * B {3}, C {4}, N {3, 5}, O {2}, P {3, 5}, S {2, 4, 6}, F Cl Br I {1}; every other symbol and '*' has none.  "v for s" is the
 * smallest normal valence >= s.
 *  - Unbracketed, not aromatic: H = v - sum1 for v for sum1; H = 0 if there is none.  The atom wants nothing.
 *  - Unbracketed, aromatic (b c n o p s, with the lists of B C N O P S; any other symbol has no list): if there is no v for sum1 the
 *    atom is AROMATIC-OVERVALENT, H = 0, it wants nothing.  Otherwise rem = v - sum1, the atom WANTS a double bond iff rem >= 1, and
 *    H = rem - (1 if it wants).  So c of benzene has H 1 and wants; the n of pyridine H 0 and wants; n with three neighbours, o, s
 *    want nothing; c(=O) of a pyridone wants nothing.
 *  - Bracket atom: H = the bracket's H count, as SMILES says.  It is never overvalent.  It wants nothing unless it is aromatic:
 *    group g = b 13, c 14, n 15, o 16, p 15, s 16 (another symbol: wants nothing), g' = g - charge, lists by g': 13 {3}, 14 {4},
 *    15 {3, 5}, 16 {2, 4, 6} (any other g': wants nothing), s' = sum1 + H; it wants iff a v for s' exists in that list and
 *    v - s' >= 1.  So [nH], [n-], [cH-] want nothing; [n+] with three neighbours, [nH+], [o+], [s+] want.
 * Per row.  W = the wanting atoms.  An EDGE is a bond entry of order 5 between two distinct atoms of W: an explicit '-' between two
 * rings is never a double bond, a bare cc bond is an edge.  Verdict, first rule that applies:
 *   MDT_MOLH_AROMATIC_OVERVALENT (1)  some atom is aromatic-overvalent; atom = the lowest such index; no search runs.
 *   MDT_MOLH_NO_KEKULE (2)            |W| is odd (zero steps).
 *   otherwise the search decides: it looks for a perfect matching of W over the edges, AND ITS ORDER IS PART OF THE DEFINITION,
 *   because its cap is.  M = the unmatched atoms of W.  M empty: verdict MDT_MOLH_OK (0).  Else u = the atom of M with the fewest
 *   neighbours in M, ties to the lowest index.  The neighbours of u in M are tried in ascending index (none: go back); each try is
 *   one STEP and removes u and that neighbour from M; a try that would be step max_steps + 1 ends the search: MDT_MOLH_UNDECIDED
 *   (3).  Going back restores the last pair (u, v) and goes on with the candidates of u above v; with nothing to restore the verdict
 *   is MDT_MOLH_NO_KEKULE.  atom = -1 for verdicts 0, 2 and 3.
 * Outputs, every word defined, zero beyond natoms.  hydrogens uint8 (R,L).  partner uint8 (R,L): 1 + the atom matched to this one
 * when the verdict is 0 and the atom is in W, else 0 -- WHICH matching is found depends on how the row is spelled; the verdict of a
 * decided row (0 or 2) does not, and neither do hydrogens, formula or verdict 1.  verdict uint8 (R), atom int32 (R).  formula int32
 * (R,13): the counts of H B C N O F P S Cl Br I, of every other symbol ('*' included), then the net formal charge; H = the sum of
 * hydrogens plus one for every atom whose symbol is H (only a bracket atom can be; it is not "other").  The formula is written for
 * every verdict.
 * What this is and is NOT.  Not RDKit's sanitisation.  Ring membership is not checked: cc is kekulisable as ethene, and an aromatic
 * atom outside any ring is judged like one inside (mdt_mol_rings counts such atoms: MDT_MOLR_AROMATIC_OUTSIDE_RING).  No aromaticity
 * perception the other way (C1=CC=CC=C1 stays as written).  No
 * radicals: an atom's free valences are filled with hydrogens.  Bracket atoms are taken at their word.  max_steps is the bound
 * every loop needs on a shared machine, and a definition, not a measurement: no row of the reference pools comes near it.
 * R == 0 launches nothing. */
#define MDT_MOLH_MAX_STEPS 4096
#define MDT_MOLH_FORMULA 13
enum mdt_molh_verdict { MDT_MOLH_OK = 0, MDT_MOLH_AROMATIC_OVERVALENT = 1, MDT_MOLH_NO_KEKULE = 2, MDT_MOLH_UNDECIDED = 3 };
int mdt_mol_hydrogens(const int32_t *natoms, const uint32_t *atoms, const int32_t *nbonds, const uint32_t *bonds, int32_t L, int32_t R,
                      int32_t max_steps, uint8_t *hydrogens, uint8_t *partner, uint8_t *verdict, int32_t *atom, int32_t *formula,
                      void *stream);

/* ------------------------------------------------------------------ */
/* Ring perception and descriptors (csrc/k_molring.hip, csrc/mdt_molring.h); additions inside ABI version 5 */
/* ------------------------------------------------------------------ */
/* Which bonds and atoms lie in a ring, how small is the smallest ring through them, and is the molecule inside the caller's bounds
 * on sixteen integer descriptors?  Everything the layers before this one answer about a row is local to an atom or a bond; "no
 * three- or four-membered ring", "no macrocycle", "at most 10 rotatable bonds", "inside Lipinski's weight / donor / acceptor
 * limits" are not.  This is a precisely defined answer on the graph of mdt_mol_graph and the hydrogens of mdt_mol_hydrogens.
 *
 * Inputs.  natoms, atoms, nbonds, bonds of mdt_mol_graph and hydrogens uint8 (R,L) of mdt_mol_hydrogens (device pointers; hydrogens
 * is required, and mdt_mol_hydrogens defines it for every verdict), R rows of width 1 <= L <= 64.  lo, hi: int32 (MDT_MOLR_DESC)
 * device pointers, both given or both NULL.  flags: uint8 (R) or NULL.  A row that is no molecule -- natoms == 0, counts outside
 * [0, L], a bond naming an atom >= natoms (the rule of mdt_mol_key) -- has all-zero outputs and flag 0.
 * The ring graph.  The simple graph on the row's atoms whose edges are the distinct unordered pairs {a, b}, a != b, named by at
 * least one bond entry, whatever the entry's order: an order outside 1..5 is an edge like any other, entries listed twice collapse
 * to one edge (C12CC12 is a row the scan accepts), an entry (a, a) is never an edge.  E = its edges, n = natoms.
 * Outputs, every word defined.
 *  bond_ring uint8 (R,L), per bond entry: for an entry (a, b), a != b: 1 + the length of a shortest path from a to b in the ring
 *   graph with the edge {a, b} removed, 0 if there is none (the bond is a bridge); for an entry (a, a): 0; 0 beyond nbonds.
 *  atom_ring uint8 (R,L), per atom: the smallest non-zero bond_ring over the entries at the atom, 0 if none, 0 beyond natoms: the
 *   size of the smallest cycle through the atom.
 *  desc int32 (R, MDT_MOLR_DESC = 16); "symbol X" means the atom's letters, in either case, bracketed or not:
 *    0 MDT_MOLR_HEAVY_ATOMS            atoms whose symbol is not H.
 *    1 MDT_MOLR_HETERO_ATOMS           heavy atoms whose symbol is not C; '*' counts.
 *    2 MDT_MOLR_DONORS                 atoms of symbol N or O with hydrogens >= 1.
 *    3 MDT_MOLR_ACCEPTORS              atoms of symbol N or O: Lipinski's N + O count.
 *    4 MDT_MOLR_ROTATABLE_BONDS        entries (a, b) of order 1 with bond_ring == 0 and a != b whose two ends each have at least 2
 *                                      distinct heavy neighbours in the ring graph and no entry of order 3 or 4 (an entry (x, x)
 *                                      included).  An entry listed twice counts twice.  AN ORDER-5 ENTRY IS NEVER ROTATABLE: a
 *                                      stated limit, which misses the axis of a biphenyl written without '-'.
 *    5 MDT_MOLR_RINGS                  E - n + components (the cycle rank).
 *    6 MDT_MOLR_RING_ATOMS             atoms with atom_ring > 0.
 *    7 MDT_MOLR_RING_BONDS             entries with bond_ring > 0.
 *    8 MDT_MOLR_SMALLEST_RING          the minimum non-zero bond_ring, 0 if there is none.
 *    9 MDT_MOLR_LARGEST_RING           the maximum bond_ring: naphthalene gives 6, not 10.
 *   10 MDT_MOLR_AROMATIC_ATOMS         atoms with descriptor bit 10.
 *   11 MDT_MOLR_AROMATIC_OUTSIDE_RING  atoms with bit 10 and atom_ring == 0: the cc that mdt_mol_hydrogens kekulises as ethene, as
 *                                      a number a bound can reject.
 *   12 MDT_MOLR_SP3_CARBONS            atoms of symbol C without bit 10 whose every entry ((x, x) included) has order 1.
 *   13 MDT_MOLR_CARBONS                atoms of symbol C.
 *   14 MDT_MOLR_COMPONENTS             the connected components of the ring graph.
 *   15 MDT_MOLR_WEIGHT                 milli-dalton: the sum over the formula slots of mdt_mol_hydrogens, H B C N O F P S Cl Br I,
 *                                      of count times 1008 10810 12011 14007 15999 18998 30974 32060 35450 79904 126904 (the
 *                                      standard atomic weights of mol_weight(), each rounded to the nearest milli-dalton); H = the
 *                                      sum of hydrogens plus the atoms of symbol H, as the formula counts it; "other" weighs 0.
 *  flags[r]: MDT_SCREEN_SUBSTRUCTURE (128) when the row is a molecule, lo and hi are given and some k has desc[k] < lo[k] or
 *   desc[k] > hi[k]; otherwise 0.  Nothing is written when flags is NULL.
 * What this is and is NOT.  Not RDKit's ring info and not an SSSR: a bond knows the smallest cycle through it, nobody lists rings,
 * and MDT_MOLR_RINGS is the cycle rank (cubane: 5, though it has six faces).  No envelope rings: the 10-ring
 * around naphthalene is nobody's smallest cycle.  No logP, so Lipinski's fourth rule is not here.  Aromaticity is as written (bit
 * 10), not perceived: C1=CC=CC=C1 has no aromatic atom.  (mdt_mol_normalize perceives it, and takes bond_ring from here.)  Donors
 * and weight rest on hydrogens as handed in.  Nothing here depends on how the row is spelled but the order of the per-entry and
 * per-atom outputs, which follow the graph row's numbering.
 * Every loop of the kernel is bounded by nbonds, natoms or both (at most nbonds searches of at most natoms levels), so there is no
 * step cap and no undecided answer.  R == 0 launches nothing.
 * Cost (131,072 mutated rows of L = 32, half of them molecules, 21 % with a ring; one MI355X, 2026-10-20): 0.0952
 * ms a call, 0.0967 ms with bounds and flags, beside 0.0649 ms for mdt_mol_hydrogens and 0.0827 ms for mdt_mol_fp on the same rows;
 * the estimate written before the first run (instruction issue, 10.1 ballot levels a molecule row) said 0.0628 ms: ratio 1.51. */
#define MDT_MOLR_DESC 16
enum mdt_molr_slot {
  MDT_MOLR_HEAVY_ATOMS = 0, MDT_MOLR_HETERO_ATOMS = 1, MDT_MOLR_DONORS = 2, MDT_MOLR_ACCEPTORS = 3, MDT_MOLR_ROTATABLE_BONDS = 4,
  MDT_MOLR_RINGS = 5, MDT_MOLR_RING_ATOMS = 6, MDT_MOLR_RING_BONDS = 7, MDT_MOLR_SMALLEST_RING = 8, MDT_MOLR_LARGEST_RING = 9,
  MDT_MOLR_AROMATIC_ATOMS = 10, MDT_MOLR_AROMATIC_OUTSIDE_RING = 11, MDT_MOLR_SP3_CARBONS = 12, MDT_MOLR_CARBONS = 13,
  MDT_MOLR_COMPONENTS = 14, MDT_MOLR_WEIGHT = 15
};
int mdt_mol_rings(const int32_t *natoms, const uint32_t *atoms, const int32_t *nbonds, const uint32_t *bonds, const uint8_t *hydrogens,
                  int32_t L, int32_t R, const int32_t *lo, const int32_t *hi, uint8_t *bond_ring, uint8_t *atom_ring, int32_t *desc,
                  uint8_t *flags, void *stream);

/* ------------------------------------------------------------------ */
/* The normal form of a graph row (csrc/k_molnorm.hip, csrc/mdt_molnorm.h); additions inside ABI version 5 */
/* ------------------------------------------------------------------ */
/* One set of graph arrays for the Kekule, the aromatic and the bracket spelling of a molecule.  mdt_mol_key, mdt_mol_fp and
 * mdt_sub_match read the graph as written, so C1=CC=CC=C1 and c1ccccc1, [CH4] and C, and the two Kekule structures of one ring are
 * different molecules to them.  This writes a graph in the same format -- atom and bond indices preserved, so natoms and nbonds are
 * reused -- in which they are one, and the three consumers take it unchanged.
 *
 * Inputs (device pointers), R rows of width 1 <= L <= 64: natoms, atoms, nbonds, bonds of mdt_mol_graph; hydrogens, partner uint8
 * (R,L) and verdict uint8 (R) of mdt_mol_hydrogens; bond_ring uint8 (R,L) of mdt_mol_rings, all for the same rows.
 * Outputs, every word defined: out_atoms uint32 (R,L), out_bonds uint32 (R,L), flags uint8 (R).
 * Rows that are not normalised.  A row that is no molecule -- natoms == 0, counts outside [0, L], a bond naming an atom >= natoms
 * (the rule of mdt_mol_key) -- has all output words 0 and flags 0.  A row with verdict != 0 has no Kekule structure to read:
 * atoms[0:natoms] and bonds[0:nbonds] are copied as written, zeros beyond, flags 0.
 * A normalised row, step by step.
 *  The Kekule view.  An entry (a, b, o) has the order k = o when o != 5.  When o == 5, k = 2 if a != b and partner[a] == 1 + b and
 *   partner[b] == 1 + a, otherwise k = 1.
 *  Per atom x.  g' = group - charge with the groups of mdt_mol_hydrogens' aromatic bracket atoms: B 13, C 14, N and P 15, O and S 16,
 *   in either case; any other symbol is ineligible, '*' and every two-letter symbol included.  dbl = the entries at x with a != b
 *   that have k == 2; sigma = the entries at x with a != b, plus hydrogens[x].  The pi electrons p(x) the atom gives to a ring:
 *    ineligible, if any entry at x (an entry (x, x) included) has k 3 or 4, or if dbl >= 2;
 *    dbl == 1 and that entry has bond_ring != 0: p = 1;
 *    dbl == 1 and that entry is no ring bond: p = 0 if x is a neutral C and the other end's symbol is N, O or S (the C of an
 *     exocyclic C=O), otherwise ineligible;
 *    dbl == 0: p = 2 if g' == 16 and sigma == 2 or g' == 15 and sigma == 3 (the O of furan, the N of pyrrole, the C of [CH-]); p = 0
 *     if g' == 13 and sigma == 3 (B, the C of [CH+]); otherwise ineligible.
 *  The rings tried.  For every entry e = (a, b) with a != b, bond_ring[e] != 0 and both ends eligible: the breadth-first search of
 *   mdt_mol_rings from a to b in the ring graph without the edge {a, b}, every atom keeping the level at which it was reached;
 *   then two walks back from b to a, at every level to the LOWEST-numbered neighbour of that level, and again to the HIGHEST.
 *   Each walk is a smallest cycle through e, hence chordless, kept as a 64-bit atom set; the two are equal when e lies in one
 *   smallest cycle.  Trying both makes the set of rings tried independent of the numbering whenever a bond lies in at most two
 *   smallest cycles, which every fusion bond of a planar ring system does.
 *  Hueckel.  A ring is aromatic when every atom in it is eligible and the sum of p over it is 2 mod 4.  Any ring size counts.
 *  The normal form.  An atom in some aromatic ring gets bit 10 set, every other atom gets it cleared.  An entry with both ends in
 *   ONE aromatic ring gets order 5 (so does an entry (x, x) at an atom of it); every other entry gets its Kekule order k.  Every
 *   atom word keeps symbol, charge and isotope as written, has the bracket bit 11 set and min(hydrogens[x], 15) in its H field.
 *   out_bonds[e] = a | b << 8 | order << 16.  Words beyond natoms / nbonds are 0.
 *  flags: MDT_MOLN_NORMALIZED (1) the row is normalised; MDT_MOLN_AROMATIC (2) at least one ring is aromatic; MDT_MOLN_CHANGED (4)
 *   some aromatic bit or bond order differs from what was written.
 * So [CH4] and C, c1ccccc1 and C1=CC=CC=C1, CC1=C(O)C=CC=C1 and CC=1C(O)=CC=CC=1 get one mdt_mol_key; the Kekule view of an aromatic
 * row normalises to the same words, bit for bit; normalising a normal form again (hydrogens and rings computed afresh) is the
 * identity.  Through the H field a pattern [CH4] of mdt_sub_match accepts the C of a normalised target, and [nH] the N of C1=CNC=C1.
 * What this is and is NOT.  Not RDKit's aromaticity model.  Rings are judged one at a time, so there are no envelope rings: azulene
 * (c1ccc2cccc2cc1: a 7-ring and a 5-ring, 10 electrons only around both) is NOT aromatic here, and RDKit says it is.  A bond in
 * three or more equally small cycles (cubane-like) may try numbering-dependent rings.  A lower-case atom outside every perceived
 * ring keeps the Kekule structure that mdt_mol_hydrogens found (cc comes out as C=C; c1ccc1 as one of its two structures).  No
 * tautomers, no charge normalisation ([O-][n+]1ccccc1 stays charged), no stereo.  bond_ring is taken at its word: an entry it calls
 * a ring bond that the search cannot close is skipped.
 * Every loop of the kernel is bounded by nbonds or natoms (at most nbonds searches of at most natoms levels, two walks of fewer
 * levels each), so there is no step cap and no undecided answer.  R == 0 launches nothing.  The cost is in DESIGN.md section 6. */
enum mdt_moln_flag { MDT_MOLN_NORMALIZED = 1, MDT_MOLN_AROMATIC = 2, MDT_MOLN_CHANGED = 4 };
int mdt_mol_normalize(const int32_t *natoms, const uint32_t *atoms, const int32_t *nbonds, const uint32_t *bonds,
                      const uint8_t *hydrogens, const uint8_t *partner, const uint8_t *verdict, const uint8_t *bond_ring, int32_t L,
                      int32_t R, uint32_t *out_atoms, uint32_t *out_bonds, uint8_t *flags, void *stream);

/* ------------------------------------------------------------------ */
/* The scaffold of a graph row (csrc/k_molscaf.hip, csrc/mdt_molscaf.h, csrc/k_screen.hip); additions inside ABI version 5 */
/* ------------------------------------------------------------------ */
/* Which ring framework is the molecule built on?  The layers above say which molecule a row is, how similar two are and what rings
 * one has; none says that two molecules are the same ring system with different side chains.  This is a precisely defined answer
 * in the spirit of Bemis and Murcko's frameworks (rings plus the linkers between them): a second set of graph arrays, in the format
 * of mdt_mol_graph, that holds the scaffold alone and that mdt_mol_key takes unchanged.
 *
 * Inputs (device pointers), R rows of width 1 <= L <= 64: natoms, atoms, nbonds, bonds of mdt_mol_graph or of mdt_mol_normalize.
 * mode: bit 0 MDT_MOLS_EXOCYCLIC (1), bit 1 MDT_MOLS_GENERIC (2); any other bit is refused before any launch.
 * Outputs, every word defined: out_natoms int32 (R), out_atoms uint32 (R,L), out_nbonds int32 (R), out_bonds uint32 (R,L),
 * atom_map uint8 (R,L), flags uint8 (R).
 * No molecule.  A row that is no molecule -- natoms == 0, a count outside [0, L], a bond naming an atom >= natoms (the rule of
 * mdt_mol_key) -- has every output word 0 and flag 0.
 * The ring graph is mdt_mol_rings': the distinct unordered pairs {a, b}, a != b, named by at least one entry, whatever the order;
 * entries listed twice collapse to one edge, an entry (a, a) is never an edge.
 * The core S.  Start from all atoms; in rounds, remove at once every atom with at most one neighbour among the atoms still present,
 *  until a round removes none.  What is left is the 2-core of the ring graph; it does not depend on the numbering.  It is the atoms
 *  on a cycle or on a path between two cycles: the rings plus the linkers, over all components.  At most ceil(n / 2) rounds remove
 *  an atom when S comes out empty (every tree loses two leaves a round), and fewer than n in any case (a tail on a ring loses one
 *  atom a round).
 * The exocyclic atoms X exist only with MDT_MOLS_EXOCYCLIC: the atoms x not in S with at least one entry (a, b, o), a != b, o == 2,
 *  whose other end is in S.  Such an x has exactly one neighbour in S and none in X, or it would be in the core.  One pass, no
 *  recursion: the =O of a ring C(=O) is kept, what hangs on it is not.  Kept = S with X; without the bit Kept = S.  If S is empty
 *  nothing is kept.
 * Kept entries: every entry with a != b and both ends kept, in its original relative order and orientation.  Entries (a, a) are
 *  dropped.
 * Renumbering: the new index x' of a kept atom x is the number of kept atoms below x.  out_bonds[e'] = a' | b' << 8 | o << 16.
 *  out_natoms / out_nbonds are the kept counts; words beyond them are 0.
 * Atom words.  Without MDT_MOLS_GENERIC an atom's word stays as written, with one exception: a bracket atom (bit 11) has its H
 *  field (bits 17..20) set to min(15, H + the sum of w(o)) over the entries at x with a != b whose other end is not kept, w(o) = o
 *  for 1 <= o <= 4 and 1 otherwise; an entry listed twice counts twice.  An unbracketed atom is unchanged, because its hydrogens
 *  are implicit.  The H rule is what lets scaffolds be compared on the normal form: the [c] of a normalised toluene becomes [cH], as
 *  in a normalised benzene.  With MDT_MOLS_GENERIC every kept atom's word is the word mdt_mol_graph writes for an unbracketed C,
 *  and every kept entry has order 1.
 * atom_map[x]: 1 + x' for a kept atom, 0 otherwise and beyond natoms.
 * flags: MDT_MOLS_MOLECULE (1) the row is a molecule; MDT_MOLS_SCAFFOLD (2) out_natoms > 0; MDT_MOLS_WHOLE (4) out_natoms ==
 *  natoms, nothing was pruned.
 * What this is and is NOT.  Not RDKit's MurckoScaffold.  Aromaticity and hydrogens are as handed in: nothing is perceived here, so
 * scaffolds of the rows as written compare spellings (c1ccccc1 and C1=CC=CC=C1 differ), scaffolds of normal forms compare
 * molecules.  With MDT_MOLS_EXOCYCLIC clear a ring C(=O) loses its O and gains two H when bracketed; on a normal form that can leave
 * an aromatic atom with an odd H count.  Stereo is ignored.  An acyclic molecule has NO scaffold: all zero, mdt_mol_key 0.
 * Applying it again with the same mode is the identity, bit for bit, in modes 0, 1 and 2; in mode 3 it is not: GENERIC rewrites the
 * exocyclic order, so a second pass drops X.  "Scaffold of the normal form" equals "normal form of the scaffold's own spelling" on
 * the hand table of the tests; it is not promised in general.
 * Every loop of the kernel is bounded by nbonds or natoms (two passes over the entries, at most natoms rounds of one ballot each),
 * so there is no step cap and no undecided answer.  R == 0 launches nothing and reads nothing.
 * Cost (131,072 mutated rows of L = 32, half of them molecules, 21 % with a scaffold; one MI355X, 2026-10-21, the
 * tree of the commit that adds k_molscaf.hip): 0.0620 ms a call beside 0.0956 ms for mdt_mol_rings on the same rows; the estimate
 * written before the first run (instruction issue, 2.2 peel rounds a molecule row) said 0.0307 ms: ratio 2.02. */
enum mdt_mols_mode { MDT_MOLS_EXOCYCLIC = 1, MDT_MOLS_GENERIC = 2 };
enum mdt_mols_flag { MDT_MOLS_MOLECULE = 1, MDT_MOLS_SCAFFOLD = 2, MDT_MOLS_WHOLE = 4 };
int mdt_mol_scaffold(const int32_t *natoms, const uint32_t *atoms, const int32_t *nbonds, const uint32_t *bonds, int32_t L,
                     int32_t R, int32_t mode, int32_t *out_natoms, uint32_t *out_atoms, int32_t *out_nbonds, uint32_t *out_bonds,
                     uint8_t *atom_map, uint8_t *flags, void *stream);
/* mdt_screen_select_similar with classes as a third way to be CLOSE: class_key uint64 (N*G), e.g. mdt_mol_key of the scaffold
 * arrays above, and max_per_class >= 1.  In step 2 a candidate with class_key != 0 is also passed over, and gets bit 16, when at
 * least max_per_class candidates kept before it carry the same class_key.  Class 0 ("no scaffold") is never counted: any number of
 * such candidates may be kept.  fp and fp_count may both be NULL (no similarity test, sim_num ignored), as may be asked of
 * mdt_screen_select_similar.  class_key == NULL: mdt_screen_select_similar itself, the same launch, max_per_class ignored. */
int mdt_screen_select_classes(const float *score, const uint64_t *key, const int32_t *packed, const int32_t *length, int32_t L,
                              int32_t N, int32_t G, const uint64_t *known_key, const int32_t *known_packed, const int32_t *known_len,
                              int32_t M, int32_t K, const int32_t *known_dist, int32_t min_novelty, int32_t min_distance,
                              const uint8_t *reject, const uint64_t *fp, const int32_t *fp_count, int32_t sim_num,
                              const uint64_t *class_key, int32_t max_per_class, uint8_t *status, int32_t *index, int32_t *count,
                              void *stream);

/* ------------------------------------------------------------------ */
/* Graph rows back to token rows (csrc/k_molwrite.hip, csrc/mdt_molwrite.h); additions inside ABI version 5 */
/* ------------------------------------------------------------------ */
/* Everything above reads SMILES; these two entries write it.  mdt_mol_rank gives every atom a visiting priority that does not
 * depend on how the row was numbered; mdt_mol_write spells graph arrays -- of mdt_mol_graph, mdt_mol_normalize, mdt_mol_scaffold or
 * any other producer -- as a token row that mdt_mol_graph reads back to the same graph, so that a scaffold or a normal form can be
 * looked at as a string and fed to the entries that take token ids.
 *
 * mdt_mol_rank.  Inputs (device pointers), R rows of width 1 <= L <= 64: the four graph arrays.  Output: priority uint64 (R,L).
 *  1. The rooted refinement of mdt_mol_key, unchanged: for every root r, lab_r[a] after the n rounds and H_r = the sum over the
 *     atoms of mix(lab_r[a]).
 *  2. The components of the ring graph of mdt_mol_rings (pairs a != b named by an entry).
 *  3. For each component c, r*(c) = the root in c with the smallest (H_r, r).
 *  4. priority[a] = lab_{r*(comp(a))}[a].
 *  5. Words beyond natoms, and rows that are no molecule by the rule of mdt_mol_key, are 0.
 *  One root per component, not one per row: with a single root two cubanes in one row would be labelled as seen from one of
 *  them, and the row would be spelled differently under renumbering.
 *
 * mdt_mol_write.  Inputs: the four graph arrays; priority uint64 (R,L) or NULL (all priorities equal: the atom index alone orders
 * the visit, "as numbered"); class_id uint8 (128), entry c the token id that stands for class c of mdt_smiles_check's class table,
 * 0: the vocabulary has no such character; the output width 1 <= W <= 128.  Outputs, every word defined: tokens int32 (R,W), the T
 * tokens at 0..T-1 and zero after; length int32 (R); token_atom uint8 (R,W); flags uint8 (R).
 * No molecule.  A row that is no molecule (the rule of mdt_mol_key; natoms == 0 included) has every output 0.
 * Not writable, MDT_MOLW_NOT_WRITABLE (8), every other output 0: an entry (a, a); a pair named by two entries; an order outside
 *  1..5; an H field (bits 17..20) above 9; a charge field (bits 12..16) outside 0..18; a letter field (bits 0..4, bits 5..9) above 26.
 * The key of atom a is (priority[a], a).  Neighbours and start atoms are taken in ascending key.
 * Pass 1, the spanning forest.  While an atom is unvisited, a depth-first walk starts at the unvisited atom of the smallest key;
 *  seq[a] counts the atoms in the order they are first reached.  At atom a its neighbours b != parent(a) are gone through in
 *  ascending key: b unvisited when its turn comes is a child of a (in that order) and is walked at once; b visited with seq[b] <
 *  seq[a]: the entry is a ring closure that OPENS at b and CLOSES at a; b visited with seq[b] > seq[a]: nothing, that closure was
 *  recorded from the other side.
 * Pass 2, the emission: the components in the order their roots were started, separated by '.'.  emit(a) writes, in this order,
 *  (1) the atom text; (2) for the closures that close at a, in ascending seq of their opening atom, that closure's number; (3) for
 *  the closures that open at a, in ascending seq of their closing atom, the bond symbol if one is needed, then the lowest free number
 *  in 1..99 (no row reaches 64); (4) for every child c in order: all but the last as '(' symbol emit(c) ')', the last as symbol
 *  emit(c).  The numbers closed at a become free only after a's own numbers are written.  A number below 10 is one digit, otherwise
 *  '%' and two digits.
 * The bond symbol: none when the order is 1 and not both atoms are aromatic (bit 10), or when it is 5 and both are; otherwise
 *  - = # $ : for the orders 1 to 5 -- the exact inverse of mdt_mol_graph's rule.  A closure's symbol stands at its opening end only.
 * The atom text.  The symbol is the first letter (upper case, lower case when bit 10 is set, '*' for 26) and, when the second field
 *  is not 0, the lower-case letter it names.  With bit 11 clear, a charge field of 9 or 0, H 0, isotope 0 and a symbol among B C N O P
 *  S F I Cl Br * b c n o p s the text is the symbol alone.  Otherwise it is '[' the isotope in decimal when it is not 0, the symbol,
 *  'H' for H == 1 or 'H' and the digit for 2..9, the charge as '+' / '-' alone for one unit or with the digit for 2..9 (field - 9;
 *  a field of 9 or 0 writes nothing), ']'.  Chirality and atom class do not exist in the graph, so none is written.
 * T is the token count.  The flags, exactly one for a molecule, in this precedence: 8 as above; MDT_MOLW_NO_VOCABULARY (4) class_id
 *  is 0 for a class the text needs; MDT_MOLW_NO_FIT (2) T > W; MDT_MOLW_WRITTEN (1) none of these.  With 4 and with 2 tokens and
 *  token_atom are all 0 and length = T.
 * token_atom is 1 + the atom a token belongs to, and 0 for '.' and beyond T: an atom's text and every ring token after it (symbol,
 *  '%', digits) belong to that atom; a bond symbol before an atom belongs to that atom; '(' and its ')' belong to the first atom
 *  inside.
 * What the writer promises.  For a written row whose unbracketed atoms pass mdt_smiles_check's valence rule, mdt_mol_graph of the
 * written tokens has status 0; its atom words equal the input's, in the order the atoms first appear in token_atom; its bonds are
 * the input's under that renumbering; hence it has the same mdt_mol_key.  With mdt_mol_rank's priority the row depends on the
 * numbering only through ties of priority that the index then breaks: on the 2,000 random spellings of the tests every graph got one
 * row, and so did every molecule of a table of symmetric ones (cubane, adamantane, pyrene, two cubanes in one row) under 24
 * renumberings each.
 * What it does NOT promise: with mdt_mol_rank's priority, a canonical form (ties are broken by index, not by search -- with
 * mdt_mol_canon's priority, below, a decided row has ONE spelling under every numbering); RDKit's canonical SMILES; stereo; a
 * preferred Kekule structure; rows wider than 128 tokens.
 * Every loop of the kernel is bounded by natoms, nbonds or W (n compares, three passes over the entries, two scalar walks of at
 * most 2 natoms and natoms + nbonds steps), so there is no step cap.  R == 0 launches nothing and reads nothing.  The cost is in
 * DESIGN.md section 6. */
enum mdt_molw_flag { MDT_MOLW_WRITTEN = 1, MDT_MOLW_NO_FIT = 2, MDT_MOLW_NO_VOCABULARY = 4, MDT_MOLW_NOT_WRITABLE = 8 };
enum { MDT_MOLW_MAX_WIDTH = 128 };
int mdt_mol_rank(const int32_t *natoms, const uint32_t *atoms, const int32_t *nbonds, const uint32_t *bonds, int32_t L, int32_t R,
                 uint64_t *priority, void *stream);
int mdt_mol_write(const int32_t *natoms, const uint32_t *atoms, const int32_t *nbonds, const uint32_t *bonds,
                  const uint64_t *priority, int32_t L, int32_t R, const uint8_t *class_id, int32_t W, int32_t *tokens,
                  int32_t *length, uint8_t *token_atom, uint8_t *flags, void *stream);

/* ------------------------------------------------------------------ */
/* The canonical atom order (csrc/k_molcanon.hip, csrc/mdt_molcanon.h); an addition inside ABI version 5 */
/* ------------------------------------------------------------------ */
/* mdt_mol_key is a hash and mdt_mol_rank breaks its ties by index; this entry SEARCHES: an individualisation-refinement tree over
 * the refinement of mdt_mol_key, the smallest relabelled graph as the answer.  Two rows are the same molecular graph exactly when
 * their canon_atoms and canon_bonds (and counts) are equal, and mdt_mol_write with this priority spells a row the same way under
 * every numbering.
 *
 * Inputs (device pointers), R rows of width 1 <= L <= 64: the four graph arrays.  A row that is no molecule by the rule of
 * mdt_mol_key has every output 0.  n = natoms, mix, ROOT and the rounds are mdt_mol_key's.
 * Refinement with marks m_0 .. m_{k-1} (distinct atoms): lab[a] = mix(atoms[a]); then lab[m_j] = mix(mix(atoms[m_j]) ^ (ROOT + j));
 *  then the n rounds of mdt_mol_key, unchanged.  With k = 1 these are the labels behind H_root.
 * Components are mdt_mol_rank's: pairs a != b named by an entry.  The search runs once per component C; all marks lie in C, and
 *  the labels come from refining the whole row.
 * A node is a mark list; the root's is empty.  The unmarked atoms of C are grouped by their label after the node's refinement (a
 *  marked atom stands alone, so a path never marks an atom twice and is at most |C| - 1 marks long).  A class is a TWIN CLASS when
 *  every member is named by exactly one entry of the row (an entry (a, a) names a twice), all those entries lead to the same other
 *  atom with the same order, and all members have the same atom word: swapping twins is an automorphism, so twin classes are never
 *  searched.  The node's TARGET is the class with the smallest label value among the classes of at least 2 members that are not
 *  twin classes.  With no target the node is a LEAF; otherwise it has one child per member of the target, the mark list extended
 *  by that member.
 * The certificate of a leaf: the atoms of C in ascending (label, index) -- only twins can tie -- take the positions 0..|C|-1; the
 *  certificate is the integer sequence |C|, the atom words in position order, the number of entries inside C, those entries as
 *  (lo position, hi position, order) in ascending order.  Certificates compare lexicographically, and the compare is on the
 *  certificates themselves, never on a hash of them: that is what makes the identity exact.
 * The canonical order of C is the position assignment of a leaf with the smallest certificate; all such leaves give the same
 *  relabelled graph, and of several the one whose positions, read in ascending atom index, are the smallest sequence is taken, so
 *  that the answer does not depend on the order in which the leaves are met.  The components are placed in ascending
 *  (certificate, lowest atom index); the canonical position of an atom is the number of atoms of the components before its own plus
 *  its position.  Every quantity in this rule is a sum or a label value that cannot depend on the numbering; ties by index happen
 *  only between twins, between leaves of one certificate and between components of one certificate, where they cannot change the
 *  relabelled graph.
 * The cap.  nodes is the number of nodes over the row's components, roots included; there is no pruning, so it is exact.  A row
 *  with nodes <= MDT_MOLC_MAX_NODES (4096, the step cap of the other searches) is decided.  Every node that is no leaf has at least
 *  2 children, so nodes < 2 x leaves: a row of at most 2,048 leaves is always decided, whatever the hash values.
 * Outputs, every word defined: priority uint64 (R,L), 1 + the canonical position, 0 beyond natoms -- mdt_mol_write's type, so that
 *  it is handed to mdt_mol_write as it is; canon_atoms uint32 (R,L), the atom words in canonical position, 0 beyond natoms;
 *  canon_bonds uint32 (R,L), the entries lo | hi << 8 | order << 16 in canonical positions, ascending in (lo, hi, order), 0 beyond
 *  nbonds; nodes int32 (R); flags uint8 (R): MDT_MOLC_CANONICAL (1); MDT_MOLC_UNDECIDED (2), the cap was passed: priority,
 *  canon_atoms and canon_bonds are all 0 and nodes is some value above the cap; 0, no molecule.
 * What it does NOT promise: RDKit's canonical SMILES or its atom order; stereo; a preferred Kekule structure (orders are compared as
 * handed in); anything for an undecided row; automorphism pruning (hexaphenylethane, 4,608 leaves, is undecided).
 * Every loop of the kernel is bounded by natoms, nbonds, 64 or the cap.  R == 0 launches nothing and reads nothing.  The cost is in
 * DESIGN.md section 6. */
enum mdt_molc_flag { MDT_MOLC_CANONICAL = 1, MDT_MOLC_UNDECIDED = 2 };
enum { MDT_MOLC_MAX_NODES = 4096 };
int mdt_mol_canon(const int32_t *natoms, const uint32_t *atoms, const int32_t *nbonds, const uint32_t *bonds, int32_t L, int32_t R,
                  uint64_t *priority, uint32_t *canon_atoms, uint32_t *canon_bonds, int32_t *nodes, uint8_t *flags, void *stream);

/* ------------------------------------------------------------------ */
/* Maximum common substructure of row pairs (csrc/k_molmcs.hip, csrc/mdt_molmcs.h); an addition inside ABI version 5 */
/* ------------------------------------------------------------------ */
/* What do these two molecules share, and where do they differ?  mdt_mol_key says same or not, mdt_mol_fp gives one number,
 * mdt_sub_map needs a fragment that is already known; this call finds the greatest connected common subgraph of two rows.
 * Inputs: the graph arrays of mdt_mol_graph (or of mdt_mol_normalize) for side A, R rows of width 1 <= LA <= 64, and for side B, RB
 * rows of width 1 <= LB <= 64, with RB == R (row by row) or RB == 1 (every A row against the one B row).  mode: bit 0
 * MDT_MCS_EXACT_ATOMS; any other bit is refused before any launch, as are widths outside 1..64, R < 0 and any other RB.  R == 0
 * launches nothing and reads nothing.
 * Usable entries.  A bond entry is USABLE when its ends differ and its order is 1..5.  A's usable entries are counted each for
 * itself, in list order (an entry listed twice counts twice).  B is read as a set: per order o an adjacency word adj_o[u] per atom.
 * A pair in which either row is no molecule -- natoms == 0, a count outside [0, width], a bond naming an atom >= natoms (the rule of
 * mdt_mol_key) -- has every output word 0.
 * Atom rule.  A atom a and B atom b are COMPATIBLE when ((atoms_a[a] ^ atoms_b[b]) & 0x7FF) == 0: symbol and aromatic bit, the mask
 * mdt_sub_match uses for an unbracketed atom.  With MDT_MCS_EXACT_ATOMS the whole words must be equal.
 * Bond rule.  Equal order.
 * Common substructure.  An injective partial map M from A atoms to B atoms of compatible pairs, and a set E of usable A entries
 * with both ends in M, each of whose images (M(a), M(b)) is a B bond of the same order; the A atoms of M must be connected through
 * E.  Its size is (|E|, |M|), compared lexicographically: bonds first.  It is the edge kind, not the induced kind: C1CC1 and CCC
 * share 2 bonds and 3 atoms.
 * Roots.  Every compatible pair (a0, b0) is a root, in ascending (a0, b0).  Root (a0, b0) searches only the A atoms >= a0, with
 * M(a0) = b0; hence every common substructure belongs to exactly one a0.
 * The walk of a root.  State: M, the used B atoms, a set X of excluded A entries, and cur, the matched entries so far.  At a node:
 *  1. If (cur, |M|) is greater than the root's best, record it (size and map).  The first record is (0, 1).
 *  2. The bound.  ub_bonds = cur + the sum over the orders o of min(ra(o), rb(o)), where ra(o) is the usable A entries of order o
 *     with both ends >= a0, not in X and not with both ends mapped, and rb(o) the B bonds of order o with not both ends used;
 *     ub_atoms = |M| + min(the unmapped A atoms >= a0, nb - |M|).  If (ub_bonds, ub_atoms) <= the root's best, or < the floor
 *     (below), return.
 *  3. Take the lowest usable A entry e = (x, y, o) in list order with both ends >= a0, e not in X, exactly one end mapped (say x)
 *     and a non-zero candidate word c = adj_o[M(x)] & compat(y) & ~used.  If there is none, return.
 *  4. For each t in c, ascending: count one STEP; set M(y) = t; cur += the usable A entries at y not in X whose other end z is
 *     mapped and whose image (M(z), t) is a B bond of their order (e itself and every closure); descend; undo.
 *  5. Then count one step, put e in X, and descend; afterwards take it out again.
 * A root about to make step MDT_MCS_MAX_STEPS + 1 is abandoned (CAPPED) and keeps its best so far.  Excluded entries are never
 * counted.  The enumeration is complete: follow any optimal (M, E), take the include branch where e is matched in it and the
 * exclude branch otherwise.
 * The floor.  Before the walks every root makes a GREEDY DESCENT: the walk above, always taking the lowest candidate of step 3,
 * never excluding and never pruning, until step 3 finds nothing; its steps are not counted.  The floor is the greatest size any
 * descent reached.  It is part of the definition, because it decides which roots reach the cap.
 * Result of a pair.  The greatest best over the roots, ties to the lowest root; the winning M is the one recorded at that best.
 * The bond mask and the bond count are then RECOUNTED from M: every usable A entry between mapped atoms whose image is a B bond of
 * its order.  For a pair with no capped root the recount equals the search's count.  No root stops or prunes because of another
 * root's progress, only because of the floor, so every word is the same under any scheduling.
 * Outputs, every word written:
 *  size int32 (R,2)        bonds, atoms.
 *  map_a uint8 (R,LA)      1 + the partner of each A atom, 0 for none and beyond natoms.
 *  bond_a uint64 (R)       bit e set for each matched A entry.
 *  steps int32 (R)         the sum over the roots, at most 4096 x 4096.
 *  out_natoms int32 (R), out_atoms uint32 (R,LA), out_nbonds int32 (R), out_bonds uint32 (R,LA), atom_map uint8 (R,LA): the
 *   common substructure as graph arrays of its own in mdt_mol_scaffold's output format, so that mdt_mol_key and mdt_mol_write take
 *   them unchanged: the kept A atoms with A's words in ascending A index, the matched entries in their order and orientation,
 *   renumbered (x' = the kept atoms below x), atom_map[x] = 1 + x' for a kept atom and 0 otherwise; words beyond the counts are 0.
 *  flags uint8 (R)         MDT_MCS_PAIR (1) both rows are molecules; MDT_MCS_COMMON (2) the result is non-empty; MDT_MCS_UNDECIDED
 *   (4) some root was capped: the result is a valid common substructure and a lower bound, like FindMCS's `canceled`;
 *   MDT_MCS_WHOLE_A (8) every atom and every usable entry of A is in the result; MDT_MCS_WHOLE_B (16) the same for B (a usable
 *   B entry is in the result when it is the image of a matched A entry).
 * What this is NOT.  Not RDKit's FindMCS: there are no ring-matches-ring options, no complete-rings option, no SMARTS result.
 * Charges, hydrogens and isotopes are ignored unless MDT_MCS_EXACT_ATOMS.  No stereo.  The result is connected, so it is ONE
 * fragment.  Aromaticity is as handed in: compare normal forms to compare molecules and not spellings.
 * A limit of the bound.  A's entries count each for itself while B is a set, so for an A row that names one pair of atoms by
 * several entries of one order (a row mdt_mol_write calls not writable; no molecule is written that way) the bound of step 2 can lie
 * under what the walk could still count, and the result, always a valid common substructure, can be smaller than the greatest one
 * without MDT_MCS_UNDECIDED.  For rows without such entries the bound is a true upper bound and a decided result is the maximum.
 * Worst case: 4,096 roots of 4,096 steps a pair, and once more for one of them (the winning map is found by running that root's
 * walk again up to the step at which its best was recorded, csrc/k_molmcs.hip). */
#define MDT_MCS_MAX_STEPS 4096
enum mdt_mcs_mode { MDT_MCS_EXACT_ATOMS = 1 };
enum mdt_mcs_flag { MDT_MCS_PAIR = 1, MDT_MCS_COMMON = 2, MDT_MCS_UNDECIDED = 4, MDT_MCS_WHOLE_A = 8, MDT_MCS_WHOLE_B = 16 };
int mdt_mol_mcs(const int32_t *a_natoms, const uint32_t *a_atoms, const int32_t *a_nbonds, const uint32_t *a_bonds, int32_t LA,
                int32_t R, const int32_t *b_natoms, const uint32_t *b_atoms, const int32_t *b_nbonds, const uint32_t *b_bonds,
                int32_t LB, int32_t RB, int32_t mode, int32_t *size, uint8_t *map_a, uint64_t *bond_a, int32_t *steps,
                int32_t *out_natoms, uint32_t *out_atoms, int32_t *out_nbonds, uint32_t *out_bonds, uint8_t *atom_map,
                uint8_t *flags, void *stream);

/* ------------------------------------------------------------------ */
/* measurement helpers (HIP events on the caller's stream)             */
/* ------------------------------------------------------------------ */
typedef struct mdt_timer mdt_timer;
mdt_timer *mdt_timer_create(int32_t max_intervals);
void mdt_timer_destroy(mdt_timer *t);
int mdt_timer_start(mdt_timer *t, void *stream); /* records the start event of the next interval */
int mdt_timer_stop(mdt_timer *t, void *stream);  /* records its stop event                         */
/* Synchronises the stop events and returns the number of intervals; ms[i] = duration of interval i. */
int32_t mdt_timer_collect(mdt_timer *t, float *ms, int32_t cap);

#ifdef __cplusplus
}
#endif
#endif /* MDT_HIP_H */
