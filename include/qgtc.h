/*
 * qgtc.h — C-ABI of libqgtc_hip.so, the MI355X (gfx950) implementation of the QGTC bit-GEMM
 * hot path. This is the drop-in boundary: plain pointers and sizes, no torch types. The
 * `QGTC` PyTorch extension (qgtc_ppopp22_amd/csrc/qgtc_torch.cpp) is a thin binding over
 * these entry points; INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * Each entry point names the reference interface it replaces (paths relative to the
 * reference checkout, YukeWang96/QGTC_PPoPP22 @ v1).
 *
 * Conventions
 *   - all pointers are DEVICE pointers on the device that is current when the call is made;
 *   - `stream` is a hipStream_t passed as void* (NULL = the legacy default stream); every
 *     call is asynchronous on that stream unless stated otherwise;
 *   - packed tensors are flat arrays of 32-bit words; element i of a packed line lives in
 *     word i>>5, bit 31-(i&31) (reference kernel.h:98,234);
 *   - "rows layout"  of an HxW matrix with b planes: [b][PAD8(H)][STEP128(W)*4] words
 *     (QGTC_device.cu:115);  "cols layout": [b][PAD128(W)][STEP128(H)*4] words
 *     (QGTC_device.cu:97), or [b][PAD8(W)][STEP128(H)*4] with output_layer (QGTC_device.cu:83);
 *   - every packed pointer must be 16-byte aligned (torch allocations are);
 *   - reads are bounds-safe: a word index >= the stated *_words reads as 0, so mis-sized or
 *     mis-laid operands (the reference reads raw memory there) can never fault;
 *   - bit widths (nbits, bit1, bit2, output_bit) must lie in [1, 32]; the reference publishes
 *     results for 1..8 only;
 *   - return value: QGTC_OK or a QGTC_E* code; qgtc_strerror() describes it. The reference
 *     printf()s and exit(-1)s instead (QGTC_device.cu:67-71).
 */
#ifndef QGTC_H
#define QGTC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QGTC_ABI_VERSION 11

enum {
    QGTC_OK = 0,
    QGTC_EINVAL = 1,   /* bad dimension / bit width / NULL pointer            */
    QGTC_ESIZE = 2,    /* output buffer smaller than the op's result          */
    QGTC_EALIGN = 3,   /* packed pointer not 16-byte aligned                  */
    QGTC_EHIP = 4,     /* HIP runtime error (see qgtc_last_hip_error())       */
    QGTC_ENODEVICE = 5 /* no gfx950 device / kernels not loadable             */
};

/* flags for qgtc_bitmm2bit */
#define QGTC_OUT_COLS 0x1u     /* pack the result in the cols layout (bitMM2Bit_col)      */
#define QGTC_NO_ZERO_SKIP 0x2u /* do not skip all-zero X tiles (result is identical)      */
#define QGTC_ZERO_JUMP 0x4u    /* qgtc_bitmm_batched: the problems carry occupancy bitmaps */
#define QGTC_ENGINE_MFMA 0x8u  /* qgtc_bitmm2bit / qgtc_bitmm2int / qgtc_bitmm_batched: expand the bit planes to
                                  int8 values and multiply on the matrix cores (bit1, bit2 <= 8; otherwise
                                  ignored). Same results; pays for wide N and several planes, not for N = 64.
                                  Grouped launches whose problems carry a one-word occupancy bitmap
                                  (K <= 8192) jump all-zero 128-row x 128-bit tiles */
#define QGTC_ENGINE_AUTO 0x10u /* let rules fitted to MI355X measurements choose between the two engines */
#define QGTC_CHAIN_DISCARD 0x40u    /* qgtc_gcn_chain_batched: the caller does not need stage_a's output itself (a hint: it is written anyway) */
/* (0x80, 0x100: flags of ABI <= 9 for a private T format between the one-launch chained pairs of rounds 2-3; that kernel family is gone -
 * qgtc_chain_transform / qgtc_chain_aggregate are the chained form) */
#define QGTC_CHAIN_ADJ_TILES 0x400u /* qgtc_chain_aggregate: the adjacencies (stage_a[b].X) are in the tile format of qgtc_adj_tiles_from_rows */
#define QGTC_CHECK_DESCRIPTORS 0x200u /* grouped entry points: a small kernel (one thread per descriptor) ahead of the product compares every DEVICE
                                  descriptor with the stated max_M / max_K / max_N (and the chaining rules of the two-stage
                                  entries) and records the first violation on the device; qgtc_last_batched_violation() reads it */

int qgtc_abi_version(void);
const char *qgtc_strerror(int code);
const char *qgtc_last_hip_error(void);

/* Shape algebra — utility.h:33-45 (STEP8/STEP128/PAD8/PAD128) and the allocation rules of
 * QGTC_device.cu:83,97,115,223,456. */
size_t qgtc_rows_words(int H, int W, int nbits);
size_t qgtc_cols_words(int H, int W, int nbits, int output_layer);

/* val2bit — replaces val2bit_cuda (QGTC_device.cu:44-130; binding QGTC_host.cpp:229-238):
 * Quantize_val (kernel.h:49-71) fused with QGTC_layer_input (kernel.h:204-242, rows layout)
 * or PackFcWeight128 (kernel.h:75-106, cols layout). x: float32 [H,W] row-major.
 * Writes every word of `out` (padding included); out_words must be >= qgtc_rows_words /
 * qgtc_cols_words. */
int qgtc_val2bit(const float *x, int H, int W, int nbits, int col_major, int output_layer,
                 uint32_t *out, size_t out_words, void *stream);

/* bit2val — replaces bit2val_cuda (QGTC_device.cu:135-206; QGTC_host.cpp:244-256):
 * UnPackFcOutput128 (kernel.h:173-201) / UnPackFcWeight128 (kernel.h:109-139).
 * out: int32 [H,W] row-major, fully written. */
int qgtc_bit2val(const uint32_t *bits, size_t bits_words, int nbits, int H, int W,
                 int col_major, int output_layer, int32_t *out, void *stream);

/* bitMM2Bit / bitMM2Bit_col — replaces bitMM2Bit_cuda (QGTC_device.cu:211-266) and
 * bitMM2Bit_col_cuda (QGTC_device.cu:441-489), i.e. kernels QGTC_layer_hidden
 * (kernel.h:245-391) and QGTC_layer_hidden_col (kernel.h:651-810):
 *   C = sum_{pa<bit1,pw<bit2} 2^(pa+pw) * popc-product(X plane pa, W plane pw)   (int32)
 *   out = pack(requant(C, output_bit))  in the rows layout, or the cols layout with
 *   QGTC_OUT_COLS.  X: rows layout of MxK with bit1 planes; W: cols layout of KxN with bit2
 *   planes (plane stride STEP128(K)*PAD128(N)*4). Writes every word of `out`. */
int qgtc_bitmm2bit(const uint32_t *X, size_t x_words, const uint32_t *W, size_t w_words,
                   int M, int K, int N, int bit1, int bit2, int output_bit,
                   uint32_t *out, size_t out_words, unsigned flags, void *stream);

/* bitMM2Int — replaces bitMM2Int_cuda (QGTC_device.cu:495-542): QGTC_layer_output_PAD8
 * (kernel.h:816-932; W plane stride STEP128(K)*PAD8(N)*4) when pad_128 == 0, else
 * QGTC_layer_output_PAD128 (kernel.h:938-1054). out: float32 [M,N] = (float)C. */
int qgtc_bitmm2int(const uint32_t *X, size_t x_words, const uint32_t *W, size_t w_words,
                   int M, int K, int N, int bit1, int bit2, int pad_128,
                   float *out, size_t out_elems, unsigned flags, void *stream);

/* bitMM2Bit_profile — replaces bitMM2Bit_cuda_profile (QGTC_device.cu:379-434): `reps`
 * back-to-back launches between two events; BLOCKS until they finish and returns the elapsed
 * milliseconds in *elapsed_ms (the reference hard-codes reps = 200 and printf()s TFLOPs). */
int qgtc_bitmm2bit_profile(const uint32_t *X, size_t x_words, const uint32_t *W, size_t w_words,
                           int M, int K, int N, int bit1, int bit2, int output_bit,
                           uint32_t *out, size_t out_words, unsigned flags, int reps,
                           float *elapsed_ms, void *stream);

/* Tile counters — replaces the `counter_global` / `counter` device globals that
 * QGTC_layer_hidden_base_cnt (kernel.h:394-512, :452) and QGTC_layer_hidden_zerojump_cnt
 * (kernel.h:516-648, :574-592) bump; per call, in the reference's 8-row x 128-bit tile units:
 *   counters[0] = STEP8(M)*STEP8(N)*STEP128(K)*bit1*bit2
 *   counters[1] = steps whose 8x128-bit X tile is non-zero (x STEP8(N)*bit2)
 * `counters` is a device pointer to two uint64; it is overwritten (not accumulated). */
int qgtc_tile_counters(const uint32_t *X, size_t x_words, int M, int K, int N, int bit1,
                       int bit2, uint64_t *counters, void *stream);

/* Batched bit-GEMM: `count` independent products in ONE launch (the Cluster-GCN / Batched-GIN
 * epoch loop of main_qgtc.py:112-155 issues one bitMM2Bit per cluster batch; on MI355X the
 * launch boundary dominates those, so the engine groups them). `problems` is a DEVICE array.
 * mode: 0 = rows-layout bits, 1 = cols-layout bits, 2 = float32 (bitMM2Int). */
typedef struct qgtc_problem {
    const uint32_t *X;
    const uint32_t *W;
    void *out;
    uint64_t x_words, w_words;
    int32_t M, K, N;
    int32_t w_lines; /* lines per W plane: PAD128(N), or PAD8(N) for bitMM2Int pad_128=0 */
    int32_t occ_words; /* 64-bit words per row tile of `occ`: ceil(STEP128(K) / 64) */
    const uint64_t *occ; /* optional (NULL = visit every k-quad): occupancy bitmap of X from
                            qgtc_tile_occupancy; zero X tiles are then neither loaded nor multiplied */
} qgtc_problem;

/* Occupancy bitmap of a rows-layout left operand, for zero-tile JUMPING in qgtc_bitmm_batched (the
 * reference only counts what jumping would save: QGTC_layer_hidden_zerojump_cnt, kernel.h:516-648).
 * Bit q of word [row_tile][q / 64] is set when the 32-row x 128-bit tile (rows 32*row_tile..+31,
 * k-quad q) has a set bit in any of the bit1 planes. qgtc_occupancy_words(M, K) 64-bit words.
 * Products are bit-identical with and without the bitmap. */
size_t qgtc_occupancy_words(int M, int K);
int qgtc_tile_occupancy(const uint32_t *X, size_t x_words, int M, int K, int bit1, uint64_t *occ,
                        size_t occ_words, void *stream);

/* The bitmaps of all problems of a grouped launch in ONE launch: every problem with a non-NULL `occ`
 * gets its bitmap written where `occ` points (occ_words must be ceil(STEP128(K) / 64)). With `stats`
 * (device pointer to two uint64) a second, one-workgroup kernel counts stats[0] = occupied and
 * stats[1] = all 32-row x 128-bit tiles and, when more than `max_fraction` of them are occupied, clears
 * the `occ` fields of the DEVICE descriptors (jumping then only costs a dependent load): the decision
 * needs no host round trip. Pass QGTC_ZERO_JUMP to qgtc_bitmm_batched either way. */
int qgtc_tile_occupancy_batched(qgtc_problem *problems, int count, int max_M, int max_K, int bit1,
                                float max_fraction, uint64_t *stats, void *stream);

/* Only the counting / clearing step, for descriptors whose bitmaps already exist (the adjacency bitmaps of
 * an epoch are shared by all its A.(...) stages). */
int qgtc_tile_occupancy_decide(qgtc_problem *problems, int count, float max_fraction, uint64_t *stats,
                               void *stream);

/* PRECONDITIONS the library cannot check (the descriptors live in device memory): max_M / max_K / max_N are at
 * least every problem's M / K / N - the grid, the split-K plan and the choice between the float32 (FP4) and int32
 * kernels are derived from them, so a larger problem than stated gets unwritten tiles or inexact sums; `occ` is
 * NULL or a valid bitmap from qgtc_tile_occupancy* for the SAME X (the matrix-core kernels follow a non-NULL `occ`
 * with or without QGTC_ZERO_JUMP). The PyTorch binding computes the maxima itself (BatchedGemm). */
int qgtc_bitmm_batched(const qgtc_problem *problems, int count, int max_M, int max_K, int max_N,
                       int bit1, int bit2, int output_bit, int mode, unsigned flags,
                       void *stream);

/* One quantised GNN layer for `count` cluster batches in ONE call - the grouped form of the reference's per-layer
 * pair (QGTC_conv.py:14-22: X.W, then A.(XW); main_qgtc.py:147-154 issues it as two extension calls per batch):
 *   stage 1   T_b   = bitMM2Bit_col(X_b, W, x_bits, w_bits, t_bits)        (cols-layout bits, written to stage1[b].out)
 *   stage 2   out_b = bitMM2Bit(A_b, T_b, a_bits, t_bits, output_bit)      mode 0: rows-layout bits
 *                   = bitMM2Int(A_b, T_b, a_bits, t_bits, pad_128 = 1)     mode 2: float32
 * stage1[b] = {X_b, W, T_b, .., M = n_b, K = f_in, N = f_out}, stage2[b] = {A_b, T_b, out_b, .., M = n_b, K = n_b,
 * N = f_out} (stage2[b].W must be stage1[b].out; w_lines = PAD128(N) in both). Runs as two grouped launches on `stream`
 * (word for word qgtc_bitmm_batched(stage1, mode 1) then qgtc_bitmm_batched(stage2, mode)); QGTC_ZERO_JUMP applies to
 * stage 2. max_* are hard preconditions as for qgtc_bitmm_batched. (Up to ABI 8 the entry also had a one-launch form
 * with in-kernel arrival counters; it measured slower and was removed - DESIGN.md appendix.) */
int qgtc_gcn_layer_batched(const qgtc_problem *stage1, const qgtc_problem *stage2, int count, int max_M, int max_K1,
                           int max_K2, int max_N, int x_bits, int w_bits, int t_bits, int a_bits, int output_bit,
                           int mode, unsigned flags, void *stream);

/* An aggregation stage and the NEXT layer's feature-transform stage in one call (main_qgtc.py:148-153: t1 = MM2Bit(bA, t0),
 * t2 = MM2Bit(t1, bW2), as the layout-correct chain issues them: the second with a cols-layout output). For every cluster
 * batch i: stage_a[i] is  out_i = requant(A_i . T_i)  (rows-layout bits, act_bits planes; A_i rows layout with a_bits
 * planes, T_i cols layout with t_bits planes), stage_xw[i] is  T'_i = requant(out_i . W')  (out_mode 1: cols-layout bits,
 * out_bits planes) or the output layer  float32(out_i . W')  (out_mode 2: [M, N'] floats, out_bits ignored; w_lines of the
 * descriptor as for qgtc_bitmm2int); W' cols layout with w_bits planes: stage_xw[i].X must be stage_a[i].out,
 * stage_xw[i].K = stage_a[i].N, stage_xw[i].M = stage_a[i].M. Word for word the result of qgtc_bitmm_batched(stage_a,
 * mode 0) followed by qgtc_bitmm_batched(stage_xw, mode out_mode), which is what it issues (ABI <= 9 had a one-launch kernel for some
 * shapes; the epoch's chained form is qgtc_chain_transform / qgtc_chain_aggregate below). QGTC_ZERO_JUMP applies to stage_a (its .occ
 * bitmaps).
 * max_* are hard preconditions as for qgtc_bitmm_batched. */
int qgtc_gcn_chain_batched(const qgtc_problem *stage_a, const qgtc_problem *stage_xw, int count, int max_M, int max_K,
                           int max_N1, int max_N2, int a_bits, int t_bits, int act_bits, int w_bits, int out_bits,
                           int out_mode, unsigned flags, void *stream);

/* Which kernel family a call takes - host only, no device work: the SAME rule functions the launchers use (qgtc_hip.hip:
 * single_route / batched_route over the predicates of launch_common.hip.h), so documentation and tests can name the kernel
 * behind a call shape (DESIGN.md section 5 is generated from these by tools/routing_table.py). mode 0 rows-layout bits, 1
 * cols-layout bits, 2 float32; flags = the engine / zero-jump flags of the launch. Returns a static string: a kernel
 * family name ("k_bitmm", "k_bitmm_fp4_one", ...) or "invalid". */
const char *qgtc_bitmm_route(int M, int K, int N, int bit1, int bit2, int output_bit, int mode, unsigned flags);
const char *qgtc_bitmm_batched_route(int max_M, int max_K, int max_N, int bit1, int bit2, int output_bit, int mode, unsigned flags);

/* Adjacency bit planes from an edge list — replaces the dense detour of sampler.py:80-101
 * (torch.sparse.FloatTensor(...).to_dense() then QGTC.val2bit(A, nbits, False, False)): the n x n
 * float matrix (5.9 MB for a 1213-node batch) is never materialised. `cells[i]` = row * W + col of
 * a DISTINCT non-zero cell (negative = skip), `counts[i]` its multiplicity (NULL = all 1); the
 * value is quantised like Quantize_val (kernel.h:39-44,49-71) and packed in the rows layout.
 * Result is word-for-word what qgtc_val2bit(dense A, rows layout) produces. */
int qgtc_pack_edges(const int64_t *cells, const int32_t *counts, size_t n_cells, int H, int W,
                    int nbits, uint32_t *out, size_t out_words, void *stream);

/* The 1-bit case of the above from the RAW edge list: src[i], dst[i] may repeat, nothing is sorted or
 * made unique first (three bitmaps count multiplicities 1, 2, >= 3 with atomic ORs; plane 0 = once or
 * three-times-and-more, the 1-bit quantiser's image of the summed matrix). `scratch`: 2 x
 * qgtc_rows_words(H, W, 1) words. Out-of-range indices are skipped and, if `bad_index` (device int) is
 * given, reported there (1) - no host round trip unless the caller wants one. */
int qgtc_pack_edge_list(const int64_t *src, const int64_t *dst, size_t n_edges, int H, int W, uint32_t *out,
                        size_t out_words, uint32_t *scratch, size_t scratch_words, int *bad_index, void *stream);

/* int8 MFMA GEMM, the comparison path — MI355X analogue of the reference's cuBLAS INT8
 * benchmark (cuBLASGemmEX/cublas_main.cu:123-172: cublasGemmEx, CUDA_R_8I in, CUDA_R_32F out).
 * C[M,N] (float32, row-major) = A[M,K] x B[K,N]; A is int8 row-major, B is passed as Bt[N,K]
 * (int8, K contiguous); int32 accumulation (v_mfma_i32_16x16x64_i8), exact. K % 16 == 0.
 * qgtc_i8gemm_profile times `reps` launches between two events like cublas_main.cu:123-172. */
int qgtc_i8gemm(const int8_t *A, const int8_t *Bt, int M, int K, int N, float *C, size_t c_elems,
                void *stream);
int qgtc_i8gemm_profile(const int8_t *A, const int8_t *Bt, int M, int K, int N, float *C,
                        size_t c_elems, int reps, float *elapsed_ms, void *stream);

/* ---- Detecting (not just documenting) the grouped entries' preconditions ------------------------------------------
 * The descriptors of qgtc_bitmm_batched / qgtc_gcn_layer_batched / qgtc_gcn_chain_batched live in device memory, so the
 * host side cannot compare them with the stated maxima (from which the grid, the split-K plan and the choice between the
 * float32 and int32 kernels are derived). With QGTC_CHECK_DESCRIPTORS in `flags` those entries first launch a
 * small kernel (one thread per descriptor) on `stream` that checks every descriptor: M <= max_M, K <= max_K, N <= max_N, all
 * positive, non-NULL 16-byte aligned operands AND outputs (the kernels store 16 bytes a lane), for the two-stage entries that
 * stage 2 really reads stage 1's output, and for the chain entries (qgtc_chain_transform / qgtc_chain_aggregate, whose stores
 * are sized from the HOST's N / N2) that every descriptor's N EQUALS the stated width - for qgtc_chain_aggregate's second
 * product the stage_xw descriptors are checked too (output pointer, N = N2, M = stage_a's M). The
 * product still runs (its results for an offending problem are unspecified, exactly as without the flag); the first
 * violation is kept in a per-device record until it is read. qgtc_epoch_plan_fill records there as well: a pool smaller
 * than qgtc_epoch_pool_layout's figure (QGTC_VIOL_POINTER) or a batch with n <= 0 (QGTC_VIOL_M) - such descriptors get M = 0,
 * which every grouped kernel skips.
 * qgtc_last_batched_violation(): waits for `stream`, returns QGTC_OK when no checked launch since the last call found a
 * violation, else QGTC_EINVAL with *problem = index of the first offending descriptor and *field = one of QGTC_VIOL_*;
 * the record is cleared. `problem` / `field` may be NULL. */
enum { QGTC_VIOL_NONE = 0, QGTC_VIOL_M = 1, QGTC_VIOL_K = 2, QGTC_VIOL_N = 3, QGTC_VIOL_POINTER = 4, QGTC_VIOL_CHAINING = 5 };
int qgtc_last_batched_violation(int *problem, int *field, void *stream);

/* val2bit of several matrices in ONE launch (the three weight matrices an epoch packs inside its clock,
 * main_qgtc.py:100-110: `QGTC.val2bit(W1.cuda(), w_bit, True, False)` x 3). `jobs` is a HOST array of at most
 * QGTC_MAX_PACK_JOBS entries; each job is exactly one qgtc_val2bit call (same words, every padding word written). */
#define QGTC_MAX_PACK_JOBS 8
typedef struct qgtc_pack_job {
    const float *x;      /* float32 [H, W] row-major, device */
    uint32_t *out;       /* packed result, device */
    uint64_t out_words;  /* capacity of `out` */
    int32_t H, W, nbits, col_major, output_layer;
    int32_t reserved;
} qgtc_pack_job;
int qgtc_val2bit_batched(const qgtc_pack_job *jobs, int n_jobs, void *stream);

/* ---- Epoch plans: the descriptors of every grouped launch of an epoch, filled ON THE DEVICE by one kernel -------------
 * The reference's epoch clock (main_qgtc.py:96-159) starts before the weights are packed and covers every per-batch
 * output allocation and launch. A grouped epoch needs, per stage, one qgtc_problem per cluster batch whose pointers chain
 * the stages' outputs; filling those on the host (75 descriptors x 6 stages, six uploads) cost more than the epoch's
 * kernels. Here the data loader's part - one qgtc_batch per cluster batch: the packed adjacency and features it built
 * (sampler.py:92-105) and the adjacency's occupancy bitmap - is made once beside the packing, and inside the clock ONE
 * launch turns `stages` (what each of the epoch's operators multiplies, main_qgtc.py:131-154) into device descriptors:
 * every stage's outputs are carved out of one pool, in batch order, each 16-byte aligned; stage s's descriptors are
 * descs[s * count .. s * count + count - 1].
 *   left / right: where an operand comes from - QGTC_SRC_A / _X / _XR / _XC of the batch, QGTC_SRC_WEIGHT + k = weights[k] (shared
 *   by all batches), QGTC_SRC_STAGE + j = the output of stage j < s of the same batch.
 *   M is the batch's node count n; K is `K`, or n when K == QGTC_DIM_NODES; N is `N`.
 *   mode / ob / pad128 as qgtc_bitmm_batched / qgtc_bitmm2int; use_occ: the descriptors carry the batch's bitmap.
 * qgtc_epoch_pool_layout (host only, no device work) gives the pool size in 32-bit words for the same arguments and,
 * optionally, every output's offset (offsets[s * count + b], in words) - the fill kernel uses the same rule. */
enum { QGTC_SRC_A = 0, QGTC_SRC_X = 1, QGTC_SRC_XR = 2, QGTC_SRC_XC = 3, QGTC_SRC_AT = 4, QGTC_SRC_WEIGHT = 16, QGTC_SRC_STAGE = 32 };
#define QGTC_DIM_NODES (-1)
#define QGTC_MAX_STAGES 8
#define QGTC_MAX_WEIGHTS 8
typedef struct qgtc_operand {
    const uint32_t *ptr;
    uint64_t words;
} qgtc_operand;
typedef struct qgtc_batch {
    qgtc_operand A;      /* adjacency, rows layout [n, n] */
    qgtc_operand X;      /* features, cols layout [n, F] (a right operand: sampler.py:99) */
    qgtc_operand XR;     /* features, rows layout [n, F] (a left operand), or {NULL, 0} */
    qgtc_operand XC;     /* features in the chain format of qgtc_chain_* (qgtc_chain_from_cols of X), or {NULL, 0} */
    qgtc_operand AT;     /* adjacency in the tile format of qgtc_chain_aggregate (qgtc_adj_tiles_from_rows of A), or {NULL, 0} */
    const uint64_t *occ; /* occupancy bitmap of A (qgtc_tile_occupancy) or NULL */
    int32_t n;           /* nodes of the batch */
    int32_t occ_words;   /* 64-bit words per row tile of `occ` */
} qgtc_batch;
typedef struct qgtc_stage {
    int32_t left, right; /* QGTC_SRC_* */
    int32_t K, N;        /* K: a number or QGTC_DIM_NODES */
    int32_t bit1, bit2, ob;
    int32_t mode;        /* 0 rows-layout bits, 1 cols-layout bits, 2 float32 */
    int32_t pad128;      /* mode 2: the right operand's planes have PAD128(N) lines (else PAD8(N)) */
    int32_t use_occ;     /* carry the batch's occupancy bitmap (left must be QGTC_SRC_A or QGTC_SRC_AT) */
    int32_t fmt;         /* mode 1 only: 0 = the cols layout, 1 = the chain format of qgtc_chain_* (qgtc_chain_words(n, N, ob) words) */
} qgtc_stage;
size_t qgtc_epoch_pool_layout(const int32_t *nodes, int count, const qgtc_stage *stages, int n_stages, uint64_t *offsets);
int qgtc_epoch_plan_fill(const qgtc_batch *batches, int count, const qgtc_stage *stages, int n_stages,
                         const qgtc_operand *weights, int n_weights, void *pool, size_t pool_words,
                         qgtc_problem *descs, void *stream);

/* ---- The chain entries: one wave per 32-row block for the whole output width (the grouped epochs at 1 .. 4 bits) ------------
 * Between the launches of a layout-correct epoch (X.W1 | A.T1 + .W2 | A.T2 + .W3 | A.T3, main_qgtc.py:147-154 with every
 * right operand in the cols layout) T is written by one launch and read by the next and by nobody else. These entries keep
 * it in a private CHAIN FORMAT - the finished matrix-core operand, qgtc_chain_words(M, N, bits) words per batch, unspecified to
 * the caller - and take the weights PRE-EXPANDED (qgtc_expand_weights, once per plan; qgtc_weight_codes_words(K, N, nbits,
 * order) words each, stated to the entry as the job's `codes_words`: a table too small for the job is QGTC_ESIZE, never a write). Word for word (after decoding) the results of the public entries; only the last call's float32 output is public.
 *   qgtc_chain_transform:  T_b = requant(X_b . W)                stage[b] = {X_b rows layout (x_bits planes, K <= 8192), -, T_b}
 *   qgtc_chain_aggregate:  out_mode 0: out_b = float32(A_b . T_b)                      stage_a[b] = {A_b, T_b, out_b}; stage_xw = NULL
 *                          out_mode 1: T'_b  = requant(requant(A_b . T_b) . W')        stage_a[b] = {A_b, T_b, -}, stage_xw[b] = {-, -, T'_b}
 *                          out_mode 2: out_b = float32(requant(A_b . T_b) . W')        stage_xw[b] = {-, -, out_b [M, N2]}
 * A_b: rows layout (or, with QGTC_CHAIN_ADJ_TILES, the tile format of qgtc_adj_tiles_from_rows), ONE plane, K <= 8192
 * (occupancy bitmaps of the descriptors are followed); t_bits / act_bits /
 * out_bits = bits of T / of the aggregate / of T': 1 .. 4, act_bits == out_bits (= the planes of the weights: a chain has one
 * width, main_qgtc.py's --bit_width), t_bits in the same format class (1 / 2 bits: one base-4 digit a nibble; 3 / 4 bits: two),
 * N, N2 <= 128; qgtc_chain_transform: out_bits 1 .. 4, x_bits <= 2 (out_bits <= 2) or <= 4 (out_bits 3 / 4).
 * ABI 11 widens both entries (bitmm_fp4_rbx.hip.h): one width of 5 .. 8 bits per chain (x_bits <= 8; N, N2 <= 128; the X . W product's
 * float32 sums must stay exact: K (2^x_bits - 1)(2^out_bits - 1) < 2^24, i.e. K <= 258 at 8 x 8 bits), or 1 .. 4 bits with up to 256
 * columns on either side (--n-hidden up to 256); qgtc_expand_weights accordingly nbits <= 8, N <= 256, K <= 256 for order 1.
 * QGTC_EINVAL outside that range: callers fall back to qgtc_gcn_chain_batched. w_codes: qgtc_expand_weights order 0 for
 * qgtc_chain_transform (the left operand arrives as packed words), order 1 for qgtc_chain_aggregate (the left operand is
 * the aggregate in the registers of the wave that computed it). max_M is a hard precondition (QGTC_CHECK_DESCRIPTORS).
 * qgtc_chain_transform's K is the K the weights were expanded for and EVERY descriptor's K must equal it: the kernel takes its
 * k-quad count and the stride of the weight tables from this argument, never from a descriptor (a larger descriptor K cannot
 * walk past the tables; QGTC_CHECK_DESCRIPTORS reports the mismatch). */
typedef struct qgtc_expand_job {
    const uint32_t *W;   /* cols layout [K, N], nbits planes of w_lines lines */
    uint32_t *codes;     /* out: qgtc_weight_codes_words(K, N, nbits, order) words (order 0: a table per k-quad of K) */
    uint64_t w_words;
    int32_t K, N, nbits, w_lines, order;
    uint32_t codes_words; /* capacity of `codes` in 32-bit words (ABI 11; was `reserved`): checked against the line above */
} qgtc_expand_job;
size_t qgtc_weight_codes_words(int K, int N, int nbits, int order);   /* (ABI 10 took (N, nbits) and left the per-k-quad factor to the caller) */
size_t qgtc_chain_words(int M, int N, int bits);   /* (ABI 11: 5 .. 8-bit values take two arrays of the 4-bit form) */
/* A cols-layout right operand (the public format: X of sampler.py:99, [H, W] with nbits <= 4 planes) in the chain format:
 * what a data loader does once beside the packing when the epoch's FIRST product is an aggregation (Batched-GIN: A . X,
 * main_qgtc.py:131). chain: qgtc_chain_words(H, W, nbits) words; nbits <= 8. */
int qgtc_chain_from_cols(const uint32_t *cols, size_t cols_words, int H, int W, int nbits, uint32_t *chain, size_t chain_words,
                         void *stream);
int qgtc_expand_weights(const qgtc_expand_job *jobs, int n_jobs, void *stream);
/* A one-plane rows-layout adjacency (the public format: bit_A of sampler.py:98, [M, K]) as 512-byte tiles
 * [32-row block][k-quad][32 rows][4 words], qgtc_adj_tiles_words(M, K) words: what a data loader makes once beside the
 * packing for qgtc_chain_aggregate(QGTC_CHAIN_ADJ_TILES). In the rows layout the 32 rows of a tile are a whole row apart, so a
 * launch that reads only the OCCUPIED tiles still pulls every cache line of A; as tiles it reads what it uses. Rows past M are
 * zero. The occupancy bitmaps (qgtc_tile_occupancy of the rows layout) describe both. */
size_t qgtc_adj_tiles_words(int M, int K);
int qgtc_adj_tiles_from_rows(const uint32_t *rows, size_t rows_words, int M, int K, uint32_t *tiles, size_t tiles_words, void *stream);
int qgtc_chain_transform(const qgtc_problem *stage, int count, int max_M, int K, int N, int x_bits, int out_bits,
                         const uint32_t *w_codes, unsigned flags, void *stream);
int qgtc_chain_aggregate(const qgtc_problem *stage_a, const qgtc_problem *stage_xw, int count, int max_M, int max_K, int N1,
                         int N2, int t_bits, int act_bits, int out_bits, int out_mode, const uint32_t *w2_codes,
                         unsigned flags, void *stream);

/* ---- The data loader's packing for ALL cluster batches of an iterator in a handful of launches -------------------------
 * sampler.py:76-106 packs every batch on its own: the batch's dense float adjacency from its edges, `QGTC.val2bit(A, 1, False,
 * False)`, `QGTC.val2bit(X, bit_width, True, False)`. Here one call packs `count` batches: per batch the 1-bit adjacency in the
 * rows layout straight from its edge list (the words qgtc_pack_edge_list gives: multiplicities 1, 2, >= 3 quantise to 1, 0, 1),
 * the features in the cols layout (the reference's bit_X) and - each optional, NULL = not wanted - the features in the rows
 * layout (left operand of the layout-correct chain's first X.W), the adjacency as 512-byte tiles (qgtc_adj_tiles_from_rows),
 * its occupancy bitmap (qgtc_tile_occupancy) and the features in the chain format (qgtc_chain_from_cols; x_bits <= 4).
 * Every output is word for word what the single-batch entry gives for that batch.
 *   `batches`: DEVICE array of `count` entries (the caller uploads it); edge indices are LOCAL to the batch (row = src,
 *   col = dst in [0, n)), int64, batch b's edges at src/dst[edge_off .. edge_off + n_edges); its features are rows
 *   feat_row .. feat_row + n - 1 of `feats` (float32, F columns, row-major).
 *   `zero` / `zero_bytes`: ONE region the call clears with one memset. It always contains `stats`; on the route WITHOUT a work
 *   buffer it must also contain every A and every scratch buffer (scratch: 2 x qgtc_rows_words(n, n, 1) words per batch - the
 *   multiplicity bitmaps of qgtc_pack_edge_list). With `work` (ABI 11; qgtc_load_work_words(count, max_n, total edges) words, 0 = not
 *   available for this iterator: max_n above 5120) the edges are bucketed by 32-row block there and every word of every A / AT / occ
 *   is written exactly once from LDS: A needs no clearing, `scratch` may be NULL. Same words either way. qgtc_load_work_words decides
 *   the route: a work buffer that cannot serve (max_n above 5120: QGTC_EINVAL; not 8-byte aligned: QGTC_EALIGN; fewer words than the
 *   fixed part of the layout: QGTC_ESIZE) is an error - the call never falls back to the route whose cleared region it was not given.
 *   max_n / max_edges: at least every batch's n / n_edges (grid sizes; hard preconditions like the grouped GEMM's maxima).
 *   stats (optional, inside `zero`): stats[0] += occupied 32-row x 128-bit adjacency tiles of all batches.
 *   bad_index (optional device int, cleared by the call): set to 1 when an edge index is out of range (such edges are skipped).
 *   formats: which of the optional feature formats ANY batch asks for (QGTC_LOAD_X_ROWS, QGTC_LOAD_X_CHAIN): a launch nobody
 *   needs is not made (the table itself lives on the device). */
#define QGTC_LOAD_X_ROWS 0x1u
#define QGTC_LOAD_X_CHAIN 0x2u
typedef struct qgtc_loader_batch {
    uint64_t edge_off, n_edges;
    uint64_t feat_row;
    int32_t n;
    int32_t reserved;
    uint32_t *A;       /* out: rows layout [n, n], one plane, qgtc_rows_words(n, n, 1) words (inside `zero` unless a work buffer is given) */
    uint32_t *scratch; /* 2 x qgtc_rows_words(n, n, 1) words (inside `zero`); NULL with a work buffer */
    uint32_t *AT;      /* out or NULL: qgtc_adj_tiles_words(n, n) words */
    uint64_t *occ;     /* out or NULL: qgtc_occupancy_words(n, n) 64-bit words */
    uint32_t *X;       /* out or NULL: cols layout [n, F], x_bits planes, qgtc_cols_words(n, F, x_bits, 0) words */
    uint32_t *XR;      /* out or NULL: rows layout [n, F], x_bits planes, qgtc_rows_words(n, F, x_bits) words */
    uint32_t *XC;      /* out or NULL: chain format, qgtc_chain_words(n, F, x_bits) words (needs X) */
} qgtc_loader_batch;
int qgtc_load_batches(const qgtc_loader_batch *batches, int count, int max_n, uint64_t max_edges, const int64_t *src,
                      const int64_t *dst, const float *feats, int F, int x_bits, void *zero, size_t zero_bytes,
                      uint64_t *stats, int *bad_index, unsigned formats, uint32_t *work, size_t work_words, void *stream);
size_t qgtc_load_work_words(int count, int max_n, uint64_t total_edges);

/* ---- Tile-compressed adjacency: a whole graph's 1-bit adjacency as its occupied tiles ------------------------------------------
 * The dense route (qgtc_pack_edge_list + qgtc_bitmm2bit) stores and streams all n^2 / 8 bytes of the adjacency and stops at
 * n = 185 363 (4 GiB per packed operand). This format keeps only the 32-row x 128-column tiles with a set bit, block-sparse like BSR:
 *   row_ptr  int64 [S32(n) + 1]       the tiles of 32-row block rb are row_ptr[rb] .. row_ptr[rb + 1] - 1; row_ptr[S32(n)] = T
 *   kquad    int32 [T]                the k-quad (128-column group) of each tile, strictly ascending within a row block
 *   tiles    32-bit words [T][32][4]  the 512-byte adjacency tile of qgtc_adj_tiles_words: row r of the block, the tile's 4 words of
 *                                     that row, element i at word i>>5, bit 31-(i&31); rows and columns past n are zero
 * S32(n) = (n + 31) / 32. Domain 1 <= n <= 2^23. The bits are exactly the words qgtc_pack_edge_list gives for the same raw edge list
 * (duplicates allowed: multiplicities 1, 2, >= 3 quantise to 1, 0, 1; self loops kept); only tiles with a set bit are stored, so the
 * format is canonical.
 *
 * Packing takes two calls, because T is known only after the first:
 *   qgtc_tiled_count   sorts the edges' cell keys in `work` (qgtc_tiled_work_words(n_edges) 32-bit words, 256-byte aligned) and
 *                      writes row_ptr; the caller reads row_ptr[S32(n)] = T and allocates kquad and tiles;
 *   qgtc_tiled_fill    writes kquad and every word of tiles from the same `work`, untouched in between.
 * Out-of-range or negative indices are skipped and, if `bad_index` (device int, cleared by the call) is given, reported there (1).
 *
 * Product (qgtc_tiledmm2bit / qgtc_tiledmm2int): requant(A_tiled . X), word for word what qgtc_bitmm2bit / qgtc_bitmm2int
 * (pad_128 = 1) give for the dense rows-layout A of the same edge list: X in the cols layout [bit2][PAD128(N)][S128(n)*4]
 * (bit2 1 .. 8, any N >= 1); out = rows layout [output_bit][PAD8(n)][S128(N)*4] (every word written; a row block without tiles
 * gives zeros) or float32 [n, N]. The int32 sums are exact for every row (deg (2^bit2 - 1) < 2^31). One kernel family whatever
 * the engine flags of the dense entries say; no work buffer. */
size_t qgtc_tiled_work_words(size_t n_edges);
int qgtc_tiled_count(const int64_t *src, const int64_t *dst, size_t n_edges, int n, int64_t *row_ptr, uint32_t *work,
                     size_t work_words, int *bad_index, void *stream);
int qgtc_tiled_fill(size_t n_edges, int n, int64_t n_tiles, int32_t *kquad, uint32_t *tiles, const uint32_t *work,
                    size_t work_words, void *stream);
int qgtc_tiledmm2bit(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const uint32_t *X,
                     size_t x_words, int N, int bit2, int output_bit, uint32_t *out, size_t out_words, void *stream);
int qgtc_tiledmm2int(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const uint32_t *X,
                     size_t x_words, int N, int bit2, float *out, size_t out_elems, void *stream);

/* ---- Transposed tiled adjacency: A^T . X from the same tiles ----------------------------------------------------------------------
 * The format above lists the tiles by row block (row = source: the product sums over out-neighbours). The in-neighbour sum A^T . X
 * reads the same tiles listed by k-quad, through a column index:
 *   col_ptr   int64 [S128(n) + 1]  the tiles of k-quad q are entries col_ptr[q] .. col_ptr[q + 1] - 1; col_ptr[S128(n)] = T
 *   col_tile  int64 [T]            the tile ids, ascending within a k-quad (so also in row-block order)
 *   col_rb    int32 [T]            the row block of each listed tile
 * The index is canonical: a function of row_ptr and kquad alone. qgtc_tiled_colindex builds it with one radix sort of the
 * (kquad, tile id) keys in `work` (qgtc_tiled_colindex_work_words(n_tiles) 32-bit words, 256-byte aligned) and one kernel; nothing is
 * read back to the host. Refusals: QGTC_EINVAL for n outside 1 .. 2^23, a negative n_tiles or a missing pointer (row_ptr, kquad,
 * col_tile, col_rb and work may be NULL when n_tiles is 0); QGTC_ESIZE for a short work buffer. The size query gives 0 for
 * n_tiles <= 0 (no buffer needed at 0) and when it cannot ask the device.
 *
 * Product (qgtc_tiledmm2bit_t / qgtc_tiledmm2int_t): requant(A_tiled^T . X), word for word what qgtc_tiledmm2bit / qgtc_tiledmm2int
 * give on the adjacency packed from the reversed edge list (qgtc_tiled_count / _fill(dst, src, n)), and so what qgtc_bitmm2bit /
 * qgtc_bitmm2int give on qgtc_pack_edge_list(dst, src, n, n, 1): multiplicities quantise per cell and survive the reversal. X, the
 * outputs, the domain (bit2 1 .. 8, output_bit 1 .. 32, any N >= 1) and the refusals are those of the forward entries; every output
 * word is written (a k-quad without tiles gives zero rows); the int32 sums are exact (in-degree (2^bit2 - 1) < 2^31). List bounds are
 * clamped to n_tiles and out-of-range row blocks skipped. The tiles are bit-transposed on the fly: no second copy is kept. */
size_t qgtc_tiled_colindex_work_words(int64_t n_tiles);
int qgtc_tiled_colindex(const int64_t *row_ptr, const int32_t *kquad, int64_t n_tiles, int n, int64_t *col_ptr, int64_t *col_tile,
                        int32_t *col_rb, uint32_t *work, size_t work_words, void *stream);
int qgtc_tiledmm2bit_t(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles, int64_t n_tiles,
                       int n, const uint32_t *X, size_t x_words, int N, int bit2, int output_bit, uint32_t *out, size_t out_words,
                       void *stream);
int qgtc_tiledmm2int_t(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles, int64_t n_tiles,
                       int n, const uint32_t *X, size_t x_words, int N, int bit2, float *out, size_t out_elems, void *stream);

/* ---- Scaled tiled products and degrees: a per-row float scale in the products' epilogue (mean aggregation) ---------------------------
 * The products above requantise the plain sum over neighbours, and requant clamps every sum above 2^output_bit: right inside a
 * Cluster-GCN batch, nearly constant on a whole graph. The scaled entries multiply each output row by a caller-given float before
 * the output is formed; with row_scale = 1 / degree that is the mean over neighbours, which stays in 0 .. 2^bit2 - 1.
 *
 * Semantics. For output row r (the adjacency's numbering), column c, the exact integer sum s = (A . X)[r, c] (A^T . X for the _t
 * entries) and row_scale float32 [n]:
 *     y[r, c] = fl32( fl32(s) * row_scale[r] )
 * fl32(s) is the int32 -> float32 conversion, round to nearest even; the product is one IEEE single multiply, round to nearest even,
 * fused with nothing. Nothing is special-cased: a row without tiles has s = 0, so a scale of inf or NaN gives NaN there. row_scale
 * may hold any float; products that are subnormal are outside the tested domain.
 *   qgtc_tiledmm2int_scaled / _t_scaled   out = y, float32 [n, N].
 *   qgtc_tiledmm2bit_scaled / _t_scaled   out = rows layout [output_bit][PAD8(n)][S128(N)*4], every word written as by the unscaled
 *                                         entries, holding the VALUE QUANTISER of y at output_bit bits - what qgtc_val2bit gives on
 *                                         y (above 2^output_bit -> 2^output_bit - 1, negative -> 1, round half to even, NaN -> 0):
 *                                         word for word qgtc_val2bit(rows layout) of the float entry's output. It is the value
 *                                         quantiser and not requant, because requant truncates and a mean must round. For
 *                                         output_bit <= 30 a scale of all ones gives the words of the unscaled entry (the quantiser
 *                                         of fl32(s) equals requant(s) there); at 31 / 32 the quantiser alone defines the output.
 * Domain, X, the variant choice by N and the refusals are those of the unscaled entries (1 <= n <= 2^23, bit2 1 .. 8, any N >= 1,
 * output_bit 1 .. 32; QGTC_ESIZE for a short out, QGTC_EALIGN as there), plus QGTC_EINVAL for a NULL row_scale. The unscaled entries
 * launch the kernels they always launched.
 *
 * Degrees (qgtc_tiled_degrees): out_deg[u] = set cells in row u, in_deg[v] = set cells in column v of the quantised adjacency
 * (multiplicities 1, 2, >= 3 count 1, 0, 1; self loops count) - the number of terms of the forward and of the transposed sum -, int32
 * [n], every element written; out_inv / in_inv float32 [n] = 1.0f / (float)deg correctly rounded, 0.0f where the degree is 0. Each of
 * the four may be NULL, not all four; a reciprocal needs its degree array (the reciprocal pass reads it: no work buffer). The
 * in-degrees are summed with integer atomics, so the result does not depend on the order in which they land; no column index needed.
 * QGTC_EINVAL for n outside 1 .. 2^23, a negative n_tiles, tiles without row_ptr / kquad / tiles, all four outputs NULL, or a
 * reciprocal without its degrees; QGTC_EALIGN for tiles off a 16-byte boundary. */
int qgtc_tiled_degrees(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, int32_t *out_deg,
                       int32_t *in_deg, float *out_inv, float *in_inv, void *stream);
int qgtc_tiledmm2bit_scaled(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n,
                            const uint32_t *X, size_t x_words, int N, int bit2, int output_bit, const float *row_scale, uint32_t *out,
                            size_t out_words, void *stream);
int qgtc_tiledmm2int_scaled(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n,
                            const uint32_t *X, size_t x_words, int N, int bit2, const float *row_scale, float *out, size_t out_elems,
                            void *stream);
int qgtc_tiledmm2bit_t_scaled(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                              int64_t n_tiles, int n, const uint32_t *X, size_t x_words, int N, int bit2, int output_bit,
                              const float *row_scale, uint32_t *out, size_t out_words, void *stream);
int qgtc_tiledmm2int_t_scaled(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                              int64_t n_tiles, int n, const uint32_t *X, size_t x_words, int N, int bit2, const float *row_scale,
                              float *out, size_t out_elems, void *stream);

/* ---- Float tiled products: the tiled adjacency times a float32 matrix, forwards and transposed -------------------------------------
 * Every product above takes its right operand as packed bit planes of at most 8 bits. These two entries aggregate a FLOAT32 matrix
 * over the same tiles: a full-precision output layer, raw input features, the A^T . dY of a backward pass.
 *
 * Semantics. X is float32 [n, N], row-major and contiguous, rows in the adjacency's numbering; out is float32 [n, N]; N >= 1, any
 * value; 1 <= n <= 2^23. For output row r let v_1 < v_2 < ... < v_d be the ids of its neighbours in ASCENDING order (qgtc_tiledmm_f32:
 * the set cells of row r; qgtc_tiledmm_f32_t: the set cells of column r; cells as the packer quantised them, self loops included).
 * Then for every column c
 *     s = +0.0f;  for k = 1 .. d:  s = fl32(s + X[v_k, c])          (IEEE single add, round to nearest even)
 *     out[r, c] = s                                  row_scale NULL
 *     out[r, c] = fl32(s * row_scale[r])             otherwise (one IEEE single multiply, fused with nothing)
 * The order is part of the contract: the result is a function of the inputs alone, identical on every launch and every kernel variant,
 * and equals the NumPy model of tests/tiled_float_model.py bit for bit. It follows that
 *   - out[r] depends on the rows of X that are neighbours of r and on no others: a NaN or an infinity in X[v] reaches exactly the rows
 *     adjacent to v (no tile is expanded to a dense 0/1 matrix, where 0 * NaN would spread it);
 *   - a row without neighbours gives +0.0f (times the scale, if any: nothing is special-cased, so 0 * inf is NaN);
 *   - when X holds integers and every partial sum stays below 2^24 in magnitude all adds are exact, and the result equals
 *     qgtc_tiledmm2int (_scaled) on the packed planes of the same integers bit for bit.
 * No float atomics are used. NaN payloads and signs are not specified. Inputs, partial sums or products that are subnormal are outside
 * the tested domain. A long row or column list (a hub) is summed serially by one row group: splitting it would change the order.
 *
 * Pointer types and the meaning of the index arrays are those of qgtc_tiledmm2int / qgtc_tiledmm2int_t. X and out must not overlap.
 * Every element of out[0 .. n*N) is written and nothing past it; list bounds are clamped to n_tiles, out-of-range k-quads / row blocks
 * and neighbour ids from n up are skipped. Refusals, before any device work: QGTC_EINVAL for n outside 1 .. 2^23, N < 1, a negative
 * n_tiles or a missing pointer (the index arrays and tiles may be NULL only when n_tiles is 0; row_scale may always be NULL);
 * QGTC_EALIGN for tiles off a 16-byte boundary or X / out / row_scale off a 4-byte boundary (rows of X are not 16-byte aligned when
 * N % 4 != 0: the kernels read and write single dwords); QGTC_ESIZE for x_elems < n * N or out_elems < n * N. */
int qgtc_tiledmm_f32(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *X,
                     size_t x_elems, int N, const float *row_scale, float *out, size_t out_elems, void *stream);
int qgtc_tiledmm_f32_t(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles, int64_t n_tiles,
                       int n, const float *X, size_t x_elems, int N, const float *row_scale, float *out, size_t out_elems,
                       void *stream);

/* Source scale (qgtc_tiledmm_f32_src / qgtc_tiledmm_f32_t_src): the arguments of the two entries above plus src_scale, float32 [n] in the
 * adjacency's numbering, a factor on the NEIGHBOUR being added:
 *     s = +0.0f;  for k = 1 .. d:  s = fl32( s + fl32( src_scale[v_k] * X[v_k, c] ) )
 *     out[r, c] = s   or   fl32(s * row_scale[r])                                       as above
 * One IEEE single multiply, then one IEEE single add, both round to nearest even and NOT fused: the two roundings per term are part of
 * the contract, so the result is bit for bit qgtc_tiledmm_f32 (_t) on the matrix fl32(src_scale[v] * X[v, c]), without that matrix
 * being formed (tests/tiled_sym_model.py). The order of the adds is unchanged. out = diag(row_scale) . A . diag(src_scale) . X; its
 * gradient with respect to X is the same product on the other direction with the two scales swapped, diag(src_scale) . A^T .
 * diag(row_scale) . dY, so a backward pass is one call of the twin entry and is specified to the bit as well. With row_scale the
 * inverse square roots of the out-degrees and src_scale those of the in-degrees (qgtc_tiled_inv_sqrt_degree) it is the GCN
 * normalisation D_out^-1/2 . A . D_in^-1/2. Nothing is special-cased: a NaN in src_scale[v] reaches exactly the rows adjacent to v,
 * 0 * inf is NaN. src_scale NULL: the call IS qgtc_tiledmm_f32 (_t), the same kernels and the same refusals. Otherwise the refusals
 * and the rules for what is written are those entries' (every element of out[0 .. n*N) and nothing past it), plus QGTC_EALIGN for
 * src_scale off a 4-byte boundary.
 *
 * qgtc_tiled_inv_sqrt_degree: out[i] = fl32( 1 / fl32( sqrt( fl32(deg[i]) ) ) ) for i < n, the square root and the division each
 * correctly rounded (np.float32(1) / np.sqrt(np.float32(deg))); 0.0f where deg[i] is 0 (or negative). deg is what qgtc_tiled_degrees
 * wrote, int32 [n]; every element of out is written with plain stores. QGTC_EINVAL for a missing pointer or n outside 1 .. 2^23,
 * QGTC_EALIGN for a pointer off a 4-byte boundary. */
int qgtc_tiledmm_f32_src(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *X,
                         size_t x_elems, int N, const float *row_scale, const float *src_scale, float *out, size_t out_elems,
                         void *stream);
int qgtc_tiledmm_f32_t_src(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                           int64_t n_tiles, int n, const float *X, size_t x_elems, int N, const float *row_scale,
                           const float *src_scale, float *out, size_t out_elems, void *stream);
int qgtc_tiled_inv_sqrt_degree(const int32_t *deg, int n, float *out, void *stream);

/* ---- Extremum tiled products: the element-wise maximum / minimum over neighbours, and its gradient -----------------------------------
 * The third reducer of message passing next to sum and mean (GraphSAGE-pool, PointNet-style layers, PNA). No scale turns a sum into a
 * maximum, so these are entries of their own. Operands, numbering, alignment and limits are those of "Float tiled products": X (dY) is
 * float32 [n, N], row-major and contiguous, rows in the adjacency's numbering; 1 <= n <= 2^23; N >= 1. `op` is 0 for max, 1 for min.
 *
 * Forward (qgtc_tiledmax_f32: the set cells of row r; qgtc_tiledmax_f32_t: the set cells of column r). For output row r let
 * v_1 < v_2 < ... < v_d be its neighbours in ascending order. For every column c
 *     d == 0:  out[r, c] = +0.0f, arg[r, c] = -1
 *     else:    a = v_1, s = X[v_1, c]
 *              for k = 2 .. d:  x = X[v_k, c];  if s is not NaN and (x is NaN or x > s  [min: x < s]):  s = x, a = v_k
 *              out[r, c] = s, arg[r, c] = a
 * out[r, c] is the word X[arg[r, c], c] bit for bit (a NaN may be any NaN): nothing is added, so nothing is rounded. The first NaN in
 * id order wins and stays; otherwise the lowest id among those attaining the extremum wins; -0 and +0 compare equal, so the lower id
 * wins and keeps its sign; infinities are ordinary values. arg is int32 [n, N] in the adjacency's numbering; it may be NULL, in which
 * case it is not written. A value in X[v] reaches only the rows adjacent to v.
 *
 * Select, the gradient (qgtc_tiledsel_f32: the set cells of row v; qgtc_tiledsel_f32_t: the set cells of column v). For output row v
 * let r_1 < r_2 < ... < r_d be its neighbours in ascending order. For every column c
 *     s = +0.0f;  for k = 1 .. d:  if arg[r_k, c] == v:  s = fl32(s + dY[r_k, c])
 *     out[v, c] = s
 * An unselected term contributes nothing, even if it is NaN or infinite (a sum that starts at +0 is never -0, so adding +0 for it
 * gives the same bits as skipping it). arg is data: any int32 is compared and never used as an address. The gradient of the forward
 * on one view with respect to X is the select on the OTHER view with that forward's arg, one launch; under ties the whole gradient
 * goes to the winner arg names. The order of the adds is the contract, as for the float products.
 *
 * Both are functions of their inputs alone - no atomics, the same bits on every launch and every kernel variant - and equal the NumPy
 * model of tests/tiled_max_model.py bit for bit. Every element of out[0 .. n*N) (and of arg[0 .. n*N) in the forward, when given) is
 * written and nothing past them; n_tiles == 0 with NULL index pointers gives +0 and -1 in the forward and +0 in the select. One launch
 * on `stream`, no host read. Refusals, before any device work, are those of qgtc_tiledmm_f32 (_t) without a row scale, and: QGTC_EINVAL
 * for op outside {0, 1} and for a NULL arg in the select entries; QGTC_EALIGN for arg off a 4-byte boundary; QGTC_ESIZE for
 * arg_elems < n * N when arg is given. */
int qgtc_tiledmax_f32(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *X,
                      size_t x_elems, int N, int op, float *out, size_t out_elems, int32_t *arg, size_t arg_elems, void *stream);
int qgtc_tiledmax_f32_t(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles, int64_t n_tiles,
                        int n, const float *X, size_t x_elems, int N, int op, float *out, size_t out_elems, int32_t *arg,
                        size_t arg_elems, void *stream);
int qgtc_tiledsel_f32(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *dY,
                      size_t dy_elems, int N, const int32_t *arg, size_t arg_elems, float *out, size_t out_elems, void *stream);
int qgtc_tiledsel_f32_t(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles, int64_t n_tiles,
                        int n, const float *dY, size_t dy_elems, int N, const int32_t *arg, size_t arg_elems, float *out,
                        size_t out_elems, void *stream);

/* ---- Attention tiled products: the softmax-weighted sum over neighbours, and its gradients ------------------------------------------
 * The reducer of GAT: out[o] = sum_k alpha[o, k] . X[k] with alpha the softmax, over o's neighbours, of the edge logits
 * leaky_relu(p[o] + q[k]). A logit is a function of two per-node scalars, so no per-edge storage exists: the weight of an edge is
 * rebuilt inside the tile walk. Operands, numbering, alignment and limits are those of "Float tiled products".
 *
 * Notation. A view is the row view (entries without _t: the neighbours of o are the set cells of row o) or the column view (_t: the
 * set cells of column o); out node o has the neighbours k_1 < k_2 < ... < k_d, ascending. p and q are float32 [n], a = negative_slope
 * is a float32 in [0, 1], X is float32 [n, N]. fl is one IEEE single operation, round to nearest even, never fused: the kernels
 * contain no fma. L(e) = e if e > 0, else fl(a * e).
 *
 * Scores. p and q must be finite, except that q[k] = -inf is allowed when a > 0 and masks neighbour k (its weight is exactly 0); a row
 * with neighbours needs one that is not masked. Outside that (NaN, +inf, a masked score with a = 0, a row whose neighbours are all
 * masked) the values are unspecified; nothing faults and nothing is read or written out of bounds. Subnormal inputs, sums and
 * products are outside the tested domain, as for the float products.
 *
 * EXP(z) for z <= 0, a fixed sequence of float32 operations (the hardware's transcendental is not used):
 *     z < -87:  0
 *     else      k = rint(fl(z * 1.44269504088896341f))                               (round half to even)
 *               r = fl( fl(z - fl(k * 0.693359375f)) - fl(k * -2.12194440e-4f) )
 *               y = 1.9875691500e-4f;  then for c in 1.3981999507e-3f, 8.3334519073e-3f, 4.1665795894e-2f, 1.6666665459e-1f,
 *                   5.0000001201e-1f:  y = fl(fl(y * r) + c)                          (the Cephes expf polynomial, Horner)
 *               y = fl( fl( fl(y * fl(r * r)) + r ) + 1 )
 *               EXP = ldexp(y, k)
 * The result is a normal number in [FLT_MIN, 1] (so ldexp is exact and adds k to the exponent field), EXP(+-0) = 1, EXP(-inf) = 0;
 * against the real exponential the error stays below 1 ulp on [-87, 0]. No subnormal is produced or relied on.
 *
 * DOT(x, y) for rows of length N, the same at every N: for j = 0 .. 63: t_j = +0, then for c = j, j + 64, ... < N:
 * t_j = fl(t_j + fl(x[c] * y[c])); then for h = 32, 16, 8, 4, 2, 1: every t_j = fl(t_j + t_(j xor h)); DOT = t_0 (all 64 are equal).
 *
 * Forward (qgtc_tiledatt_f32 / _t with backward = 0; att_own = p, att_nbr = q, shift = M). For each out node o
 *     M[o]   = element [o, 0] of qgtc_tiledmax_f32 (_t) on q as an [n, 1] matrix, op 0: the caller runs that launch first. L and the
 *              rounded add are monotone, so the largest logit of o is L(fl(p[o] + M[o])) exactly; +0 when d = 0.
 *     m[o]   = L(fl(p[o] + M[o]))
 *     den = +0, s[c] = +0;  for k = k_1 .. k_d:  e = fl(p[o] + q[k]);  z = fl(L(e) - m[o]) (<= 0);  w = EXP(z);
 *                                                den = fl(den + w);  s[c] = fl(s[c] + fl(w * X[k, c]))
 *     inv[o] = fl(1 / den) if d > 0 (the maximal neighbour has w = 1, so den >= 1), else 0
 *     out[o, c] = fl(s[c] * inv[o])
 * A row without neighbours gives out = +0, m = L(p[o]), inv = 0. m and inv (float32 [n]) are outputs and feed the backward.
 *
 * Backward. With dY, the forward's Y, m and inv, D[o] = DOT(dY[o], Y[o]) (qgtc_rowdot_f32), and per edge, recomputed with the same
 * bits, e = fl(p[o] + q[k]), w = EXP(fl(L(e) - m[o])), alpha = fl(w * inv[o]):
 *     dX[k, c]  on the OTHER view, over the neighbours o of k ascending: s = fl(s + fl(alpha * dY[o, c]))
 *               (qgtc_tiledatt_f32 / _t with backward = 1: X = dY, att_own = q, att_nbr = p, shift = m, inv read, m unused)
 *     u         = fl(alpha * fl(DOT(dY[o], X[k]) - D[o]));  if not e > 0:  u = fl(a * u)
 *     dp[o]     the fold of u over k ascending on the forward's view
 *               (qgtc_tiledatt_grad_f32 / _t, nbr_owns = 0: A = dY, B = X, att_own = p, att_nbr = q)
 *     dq[k]     the fold of u over o ascending on the other view
 *               (qgtc_tiledatt_grad_f32 / _t, nbr_owns = 1: A = X, B = dY, att_own = q, att_nbr = p; m, inv, D are the neighbour's)
 * The derivative of L at e = 0 exactly (+0 or -0) is therefore a, the negative slope, as L itself takes the fl(a * e) branch there:
 * the convention of torch.nn.functional.leaky_relu, whose derivative is 1 for e > 0 and a otherwise.
 * Every fold starts from +0 and adds one term at a time. No atomics: all results are functions of the inputs alone, the same bits on
 * every launch and every kernel variant, and equal the NumPy model of tests/tiled_attn_model.py bit for bit.
 *
 * Every element of out (forward / backward: [n, N]; gradient and row dot: [n]), and of m and inv in the forward, is written and
 * nothing past them; n_tiles == 0 with NULL index pointers is an adjacency without edges. One launch on `stream` each, no host read.
 * Refusals, before any device work, in the order of qgtc_tiledmm_f32: QGTC_EINVAL for its cases, a missing vector (att_own, att_nbr,
 * shift, inv, m where it is written; B, m, inv, D in the gradient), backward / nbr_owns outside {0, 1} and a slope outside [0, 1] or
 * NaN; QGTC_EALIGN for a pointer off its boundary (4 bytes for all floats); QGTC_ESIZE for x_elems (ab_elems: A and B each) < n * N,
 * out_elems < n * N (gradient and row dot: < n). */
int qgtc_tiledatt_f32(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *X,
                      size_t x_elems, int N, const float *att_own, const float *att_nbr, float negative_slope, int backward,
                      const float *shift, float *m, float *inv, float *out, size_t out_elems, void *stream);
int qgtc_tiledatt_f32_t(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles, int64_t n_tiles,
                        int n, const float *X, size_t x_elems, int N, const float *att_own, const float *att_nbr, float negative_slope,
                        int backward, const float *shift, float *m, float *inv, float *out, size_t out_elems, void *stream);
int qgtc_tiledatt_grad_f32(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *A,
                           const float *B, size_t ab_elems, int N, const float *att_own, const float *att_nbr, float negative_slope,
                           int nbr_owns, const float *m, const float *inv, const float *D, float *out, size_t out_elems, void *stream);
int qgtc_tiledatt_grad_f32_t(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                             int64_t n_tiles, int n, const float *A, const float *B, size_t ab_elems, int N, const float *att_own,
                             const float *att_nbr, float negative_slope, int nbr_owns, const float *m, const float *inv, const float *D,
                             float *out, size_t out_elems, void *stream);
int qgtc_rowdot_f32(const float *A, const float *B, size_t ab_elems, int n, int N, float *out, size_t out_elems, void *stream);

/* ---- Edge dropout: a random subgraph per launch, decided inside the tile walk ------------------------------------------------------
 * DropEdge / neighbourhood dropout for every float product above without a second adjacency: whether cell (i, j) of A survives is a
 * pure function of (i, j, seed), rebuilt in the kernels as the tiles are decoded. i is A's row and j A's column in the adjacency's own
 * numbering; on the transposed view the cell is still A's, so a backward on the other view sees exactly the forward's subgraph. All
 * arithmetic is uint32 and wraps:
 *     mix32(x):  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16
 *     k0 = seed & 0xffffffff,  k1 = seed >> 32,  K = mix32(k0) + k1
 *     R(i) = mix32(i ^ k0),  C(j) = mix32(j ^ k1) + 0x9E3779B9,  H(i, j, seed) = mix32((R(i) ^ C(j)) + K)
 *     kept(i, j)  <=>  H(i, j, seed) >= threshold          (threshold = floor(rate * 2^32), computed in double, for a drop rate in [0, 1))
 * qgtc_edge_kept returns kept(i, j) (1 or 0) on the host, with the functions the kernels run; it needs no device.
 *
 * Masking is dropping: each _drop entry returns bit for bit what its parent returns on an adjacency packed from the kept cells only
 * (same numbering, so the folds run over the kept neighbours in ascending id order); a dropped neighbour's row is never loaded. Nothing
 * is rescaled. A row that loses every neighbour is a row without neighbours: +0, arg = -1, inv = 0 and m as documented above.
 * threshold 0 keeps every cell and gives the parent's bits. Each entry is its parent's signature with `threshold, seed` before `stream`
 * and the parent's refusals in the parent's order (qgtc_tiledmm_f32_drop / _t_drop: qgtc_tiledmm_f32_src's, with both scales nullable).
 * The selects (qgtc_tiledsel_f32 / _t) need no mask: arg names kept neighbours only. In the attention forward `shift` must be the MASKED
 * maximum of att_nbr (qgtc_tiledmax_f32_drop / _t_drop with N = 1 and the same threshold and seed): with the unmasked one the weights'
 * sum may fall below 1 and inv overflow. The backward and both score gradients take the forward's (threshold, seed). */
int qgtc_edge_kept(uint32_t i, uint32_t j, uint64_t seed, uint32_t threshold);
int qgtc_tiledmm_f32_drop(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *X,
                          size_t x_elems, int N, const float *row_scale, const float *src_scale, float *out, size_t out_elems,
                          uint32_t threshold, uint64_t seed, void *stream);
int qgtc_tiledmm_f32_t_drop(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                            int64_t n_tiles, int n, const float *X, size_t x_elems, int N, const float *row_scale,
                            const float *src_scale, float *out, size_t out_elems, uint32_t threshold, uint64_t seed, void *stream);
int qgtc_tiledmax_f32_drop(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *X,
                           size_t x_elems, int N, int op, float *out, size_t out_elems, int32_t *arg, size_t arg_elems,
                           uint32_t threshold, uint64_t seed, void *stream);
int qgtc_tiledmax_f32_t_drop(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                             int64_t n_tiles, int n, const float *X, size_t x_elems, int N, int op, float *out, size_t out_elems,
                             int32_t *arg, size_t arg_elems, uint32_t threshold, uint64_t seed, void *stream);
int qgtc_tiledatt_f32_drop(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *X,
                           size_t x_elems, int N, const float *att_own, const float *att_nbr, float negative_slope, int backward,
                           const float *shift, float *m, float *inv, float *out, size_t out_elems, uint32_t threshold, uint64_t seed,
                           void *stream);
int qgtc_tiledatt_f32_t_drop(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                             int64_t n_tiles, int n, const float *X, size_t x_elems, int N, const float *att_own, const float *att_nbr,
                             float negative_slope, int backward, const float *shift, float *m, float *inv, float *out, size_t out_elems,
                             uint32_t threshold, uint64_t seed, void *stream);
int qgtc_tiledatt_grad_f32_drop(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n,
                                const float *A, const float *B, size_t ab_elems, int N, const float *att_own, const float *att_nbr,
                                float negative_slope, int nbr_owns, const float *m, const float *inv, const float *D, float *out,
                                size_t out_elems, uint32_t threshold, uint64_t seed, void *stream);
int qgtc_tiledatt_grad_f32_t_drop(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                                  int64_t n_tiles, int n, const float *A, const float *B, size_t ab_elems, int N, const float *att_own,
                                  const float *att_nbr, float negative_slope, int nbr_owns, const float *m, const float *inv,
                                  const float *D, float *out, size_t out_elems, uint32_t threshold, uint64_t seed, void *stream);

/* ---- Node masks: induced subgraphs on the whole-graph adjacency, without re-packing ------------------------------------------------------
 * A node set is a BITMAP of int32 words [S128(n) * 4] in the bit order of a tile row: node i at word i >> 5, bit 31 - (i & 31). The
 * length is a whole number of k-quads, so the four words beside a tile are one 16-byte aligned read; the bitmap is in the adjacency's
 * own numbering. qgtc_node_bitmap builds it on the device from byte flags [n] (non-zero = member; one thread a word, plain stores,
 * deterministic), with the bits at positions >= n and the pad words zero. The kernels ignore such bits anyway: their v < n / row < n
 * guards stay. QGTC_EINVAL for a NULL pointer or n outside 1 .. 2^23, QGTC_EALIGN for words off a 16-byte boundary, QGTC_ESIZE for
 * words_len < S128(n) * 4.
 *
 * On a view (the _t entries: A^T) the _nodes entries take row_mask and nbr_mask, each a bitmap or NULL = all nodes, relative to the
 * view like row_scale / src_scale:
 *   - output row o is computed iff o is in row_mask; otherwise it holds exactly what a row without neighbours holds: +0 in every
 *     column (times row_scale[o], as that row would), arg -1, and the attention statistics of a neighbourless row;
 *   - neighbour k of a computed row takes part iff k is in nbr_mask; a neighbour outside it is never queued and its row of X (and its
 *     src_scale) is never loaded.
 * Everything else - ascending-id order, one IEEE add per term, the unfused source scale, the tie and NaN rules of max / min - is unchanged, so the result is bit for bit the
 * unmasked entry on an adjacency packed from the edges whose output-row end lies in row_mask and whose neighbour end lies in nbr_mask.
 * The backward of Y = mask(A) . X on the other view takes the two masks swapped (as it takes the two scales swapped). All-ones masks, or
 * two NULLs, give the plain entry's bits. A workgroup none of whose output rows is in row_mask reads no index and no tile.
 * Each entry is its _drop twin's signature with (row_mask, nbr_mask, mask_words) in place of (threshold, seed), and its refusals in its
 * order; then QGTC_ESIZE for a mask with mask_words < S128(n) * 4 and QGTC_EALIGN for a mask off a 16-byte boundary, all before any
 * device work. Degrees of the masked graph need no entry: they are the masked N = 1 product of a column of ones (exact: n <= 2^23).
 * The extremum: a row outside row_mask holds +0 and arg -1; the selects (qgtc_tiledsel_f32 / _t) need no mask, because arg names
 * participating neighbours only. The attention product: a row outside row_mask holds +0, inv = 0 and m as a row without neighbours;
 * EXP and the softmax run over the participating neighbours, so in the forward `shift` must be the MASKED maximum of att_nbr
 * (qgtc_tiledmax_f32_nodes / _t_nodes with N = 1 and the same masks). grad_own runs on the forward's view with the forward's masks; the
 * backward product and grad_nbr run on the other view with the two masks swapped.
 *
 * qgtc_tiled_inv_degree: out[i] = 1.0f / (float)deg[i] correctly rounded, 0.0f where deg[i] is 0 - the reciprocal pass of
 * qgtc_tiled_degrees on its own (the same kernel), for the degrees of a masked graph. Refusals as qgtc_tiled_inv_sqrt_degree's. */
int qgtc_tiled_inv_degree(const int32_t *deg, int n, float *out, void *stream);
int qgtc_node_bitmap(const uint8_t *flags, int n, uint32_t *words, size_t words_len, void *stream);
int qgtc_tiledmm_f32_nodes(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *X,
                           size_t x_elems, int N, const float *row_scale, const float *src_scale, float *out, size_t out_elems,
                           const uint32_t *row_mask, const uint32_t *nbr_mask, size_t mask_words, void *stream);
int qgtc_tiledmm_f32_t_nodes(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                             int64_t n_tiles, int n, const float *X, size_t x_elems, int N, const float *row_scale,
                             const float *src_scale, float *out, size_t out_elems, const uint32_t *row_mask, const uint32_t *nbr_mask,
                             size_t mask_words, void *stream);
int qgtc_tiledmax_f32_nodes(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *X,
                            size_t x_elems, int N, int op, float *out, size_t out_elems, int32_t *arg, size_t arg_elems,
                            const uint32_t *row_mask, const uint32_t *nbr_mask, size_t mask_words, void *stream);
int qgtc_tiledmax_f32_t_nodes(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                              int64_t n_tiles, int n, const float *X, size_t x_elems, int N, int op, float *out, size_t out_elems,
                              int32_t *arg, size_t arg_elems, const uint32_t *row_mask, const uint32_t *nbr_mask, size_t mask_words,
                              void *stream);
int qgtc_tiledatt_f32_nodes(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *X,
                            size_t x_elems, int N, const float *att_own, const float *att_nbr, float negative_slope, int backward,
                            const float *shift, float *m, float *inv, float *out, size_t out_elems, const uint32_t *row_mask,
                            const uint32_t *nbr_mask, size_t mask_words, void *stream);
int qgtc_tiledatt_f32_t_nodes(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                              int64_t n_tiles, int n, const float *X, size_t x_elems, int N, const float *att_own, const float *att_nbr,
                              float negative_slope, int backward, const float *shift, float *m, float *inv, float *out, size_t out_elems,
                              const uint32_t *row_mask, const uint32_t *nbr_mask, size_t mask_words, void *stream);
int qgtc_tiledatt_grad_f32_nodes(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n,
                                 const float *A, const float *B, size_t ab_elems, int N, const float *att_own, const float *att_nbr,
                                 float negative_slope, int nbr_owns, const float *m, const float *inv, const float *D, float *out,
                                 size_t out_elems, const uint32_t *row_mask, const uint32_t *nbr_mask, size_t mask_words, void *stream);
int qgtc_tiledatt_grad_f32_t_nodes(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                                   int64_t n_tiles, int n, const float *A, const float *B, size_t ab_elems, int N, const float *att_own,
                                   const float *att_nbr, float negative_slope, int nbr_owns, const float *m, const float *inv,
                                   const float *D, float *out, size_t out_elems, const uint32_t *row_mask, const uint32_t *nbr_mask,
                                   size_t mask_words, void *stream);

/* ---- Edge values: a float32 per stored cell of the tiled adjacency, the weighted sum and the per-edge dot (SDDMM) ----------------------
 * A weighted graph is a tiled adjacency plus a float32 vector `values` of n_values = nnz elements, nnz the number of set bits of the
 * tiles. The SLOT of cell (i, j) is its rank when the set bits are listed by tile id, then tile row, then column ascending (MSB first
 * within a word, as the decode goes). It depends on the tiles alone and not on the view, so one array serves A and A^T. Two index arrays
 * make a slot computable from a tile row's four words:
 *   val_ptr  int64 [T + 1]   the exclusive prefix sum of the tiles' bit counts (val_ptr[T] = nnz);
 *   val_row  int16 [T, 32]   within tile t, the set bits in the rows above r (at most 31 * 128 = 3968);
 *   slot(t, r, c) = val_ptr[t] + val_row[t][r] + popcount(the bits of row r before column c).
 * That is 72 bytes beside a 512-byte tile. Slots are held in 32 bits inside the kernels: every entry that takes n_values refuses n_values > 2^31 - 1
 * (QGTC_EINVAL).
 *
 * qgtc_tiled_value_index writes counts[t] = the set bits of tile t (int64 [T]) and val_row. The scan of counts into val_ptr is the
 * CALLER'S (an exclusive prefix sum with the total appended: torch.cumsum in the Python package). QGTC_EINVAL for a negative n_tiles or
 * a missing pointer (all three may be NULL when n_tiles is 0), QGTC_EALIGN for tiles off 16 bytes, counts off 8 or val_row off 2.
 * qgtc_tiled_edge_slots: slot[e] (int64 [n_edges]) of the cell (src[e], dst[e]) - a binary search of kquad within row block src >> 5 for
 * k-quad dst >> 7, then the cell's bit -, or -1 where the cell is not set (multiplicity 2 quantised it to 0, or the edge is not in the
 * graph) or an id lies outside [0, n): nothing is read outside the arrays. Ids are the adjacency's own numbering.
 * qgtc_tiled_edge_endpoints: the inverse, row[s] / col[s] (int32 [n_values]) = the cell of slot s, in the adjacency's numbering; a slot
 * from n_values up is not written.
 * Both: QGTC_EINVAL for n outside 1 .. 2^23, a negative n_tiles, tiles without row_ptr / kquad / tiles / val_ptr / val_row or a missing
 * src / dst / slot (row / col) when there are edges (values); QGTC_EALIGN for tiles off 16 bytes, val_ptr / src / dst / slot off 8,
 * row / col off 4, val_row off 2.
 *
 * qgtc_tiledmm_f32_edge / _t_edge: the arguments of qgtc_tiledmm_f32 / _t, then (val_ptr, val_row, values, n_values):
 *   out[i] = row_scale[i] . sum over i's neighbours j of the view, ASCENDING, of fl(values[slot of the cell] * X[j])
 * - the term of the source scale, one IEEE multiply, then one IEEE add, never fused; only the factor's address is new. With all values
 * 1.0 the result is the plain entry's bits; with values[s] = c[col of s] it is qgtc_tiledmm_f32_src with src_scale = c, and with
 * values[s] = c[row of s] it is qgtc_tiledmm_f32_t_src. Refusals as qgtc_tiledmm_f32's in its order, with QGTC_EINVAL also for missing
 * val_ptr / val_row / values when n_tiles > 0 and QGTC_EALIGN also for values off 4 bytes, val_ptr off 8, val_row off 2. A slot outside
 * [0, n_values) - a foreign index - reads nothing and counts as 0.
 *
 * qgtc_tiled_sddmm_f32: out[slot(i, j)] = DOT(A[i], B[j]) for every stored cell (i, j) of A_tiled, DOT exactly that of "Attention tiled
 * products" (64 strided partial sums t_l over the columns l, l + 64, ..., each from +0 by one unfused multiply and add a column, then
 * the xor butterfly h = 32 .. 1). Every slot below n_values is written exactly once with a plain store; no atomics. Only the row view
 * exists: on A^T the cell is the same and the operands swap. It is the gradient for `values` of the weighted sum (A = diag(row_scale) . dY,
 * B = X), a link score, and the building block of dot-product attention. Refusals in the same order: QGTC_EINVAL as above with A, B, out;
 * QGTC_EALIGN for A / B / out off 4 bytes; QGTC_ESIZE for ab_elems (A and B each) < n * N. */
int qgtc_tiled_value_index(const uint32_t *tiles, int64_t n_tiles, int64_t *counts, int16_t *val_row, void *stream);
int qgtc_tiled_edge_slots(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n,
                          const int64_t *val_ptr, const int16_t *val_row, const int64_t *src, const int64_t *dst, size_t n_edges,
                          int64_t *slot, void *stream);
int qgtc_tiled_edge_endpoints(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n,
                              const int64_t *val_ptr, const int16_t *val_row, int32_t *row, int32_t *col, size_t n_values, void *stream);
int qgtc_tiledmm_f32_edge(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *X,
                          size_t x_elems, int N, const float *row_scale, float *out, size_t out_elems, const int64_t *val_ptr,
                          const int16_t *val_row, const float *values, size_t n_values, void *stream);
int qgtc_tiledmm_f32_t_edge(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                            int64_t n_tiles, int n, const float *X, size_t x_elems, int N, const float *row_scale, float *out,
                            size_t out_elems, const int64_t *val_ptr, const int16_t *val_row, const float *values, size_t n_values,
                            void *stream);
int qgtc_tiled_sddmm_f32(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *A,
                         const float *B, size_t ab_elems, int N, const int64_t *val_ptr, const int16_t *val_row, float *out,
                         size_t n_values, void *stream);

/* ---- Edge softmax: a vector of per-edge logits normalised over each node's neighbourhood, and its gradient ----------------------------
 * `logits`, `alpha` and `g` are float32 [n_values] in SLOT order ("Edge values"); slots depend on the tiles alone, so the same vectors
 * serve both views. On the row view the OWNER of cell (i, j) is row i; on the column view (_t) it is column j. An owner's cells are
 * taken in ascending id of the other end - ascending neighbour id, as in every float product. EXP is the exponential of "Attention
 * tiled products"; no operation is fused.
 *   forward, for an owner o with cells k = 1 .. d in that order:
 *     m[o]   = l_1, then m = l_k > m ? l_k : m for k = 2 .. d (the first of equal values wins: the bits of m are specified);
 *     w_k    = EXP(fl(l_k - m[o]));
 *     den    = the in-order fold from +0 of w_k, one float32 add each;
 *     inv[o] = den > 0 ? 1 / den : 0, IEEE division (the expression of the attention forward);
 *     alpha[slot_k] = fl(w_k * inv[o]).
 *   An owner without cells writes nothing to alpha and has m = +0 and inv = 0. l_k = -inf gives alpha = +0 for that edge, provided the
 *   owner has one finite logit. A NaN or +inf logit gives unspecified values for that owner's cells only and touches no memory outside
 *   the arrays; the same holds for an owner whose logits are all -inf. `m` and `inv` (float32 [n]) are optional outputs (NULL: not
 *   wanted); when given, all n elements are written, also when there are no tiles.
 *   gradient, given alpha and g = dL/dalpha:
 *     t_k  = fl(alpha_k * g_k);   S[o] = the in-order fold from +0 of t_k;   out[slot_k] = fl(alpha_k * fl(g_k - S[o])).
 * Every slot below n_values is written exactly once with a plain store, on either view; no atomics. A slot outside [0, n_values) - a
 * foreign index - is never dereferenced: the cell is skipped.
 * Refusals before any device work: QGTC_EINVAL for n outside 1 .. 2^23, a negative n_tiles, tiles without the view's index arrays /
 * tiles / val_ptr / val_row, values without logits / alpha (alpha / g / out), or n_values > 2^31 - 1; then QGTC_EALIGN for tiles off
 * 16 bytes, val_ptr off 8, val_row off 2 or a float array off 4. n_tiles == 0 or n_values == 0 returns QGTC_OK after filling m / inv
 * (where given) with +0. */
int qgtc_tiled_edge_softmax_f32(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n,
                                const int64_t *val_ptr, const int16_t *val_row, const float *logits, float *alpha, size_t n_values,
                                float *m, float *inv, void *stream);
int qgtc_tiled_edge_softmax_f32_t(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                                  int64_t n_tiles, int n, const int64_t *val_ptr, const int16_t *val_row, const float *logits,
                                  float *alpha, size_t n_values, float *m, float *inv, void *stream);
int qgtc_tiled_edge_softmax_grad_f32(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n,
                                     const int64_t *val_ptr, const int16_t *val_row, const float *alpha, const float *g, float *out,
                                     size_t n_values, void *stream);
int qgtc_tiled_edge_softmax_grad_f32_t(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                                       int64_t n_tiles, int n, const int64_t *val_ptr, const int16_t *val_row, const float *alpha,
                                       const float *g, float *out, size_t n_values, void *stream);

/* ---- Node reordering: ids that keep a tiled adjacency compact --------------------------------------------------------------------
 * The tiled format only pays off when a node's neighbours have nearby ids: under random ids nearly every edge occupies a tile of its
 * own (512 bytes an edge). qgtc_reorder_nodes renumbers the nodes on the device from a raw edge list with any ids:
 *   neighbour entries  every valid edge s -> d with s != d adds the entries (s, d) and (d, s); duplicates count once each; self loops
 *                      and out-of-range edges add nothing (the latter are reported through `bad_index`, as in qgtc_tiled_count);
 *   sweeps             label[x] = x, then sweeps t = 0 .. sweeps - 1 (all on the labels before the sweep): a node x with entries and
 *                      (x + t) even proposes the label l most of its entries' other ends carry, ties to the smallest
 *                      mix32(l ^ (0x9E3779B9 (t + 1) mod 2^32)) (lowbias32); every other node proposes its own label. A proposal
 *                      is taken when it is the current label or at most `cap` nodes propose it (a soft cap). The sweeps stop after
 *                      two in a row that change no label;
 *   output             perm (int64 [n]) = the nodes sorted by (label, id), perm[new] = old; rank (int64 [n], may be NULL) its
 *                      inverse, rank[old] = new. With no edges or sweeps = 0 both are the identity.
 * The result is deterministic (integer counts; it does not depend on the order in which atomics land) and equals the NumPy model in
 * tests/reorder_model.py element for element. Relabelled edges (rank[src], rank[dst]) packed with qgtc_tiled_count / _fill give the
 * adjacency in the new numbering; the products then read X and give their output in that numbering.
 * Domain: 1 <= n <= 2^23, 0 <= sweeps <= 64, cap >= 1. `work`: qgtc_reorder_work_words(n, n_edges) 32-bit words, 256-byte aligned
 * (unused and may be NULL without edges; the size query needs the device: 0 when it fails or n is outside the domain). QGTC_EINVAL
 * for a domain violation, a missing perm, or edges without src, dst or work; QGTC_ESIZE for a work buffer that is too small. The host
 * queues every launch without reading anything back. */
size_t qgtc_reorder_work_words(int n, size_t n_edges);
int qgtc_reorder_nodes(const int64_t *src, const int64_t *dst, size_t n_edges, int n, int sweeps, int cap, int64_t *perm,
                       int64_t *rank, uint32_t *work, size_t work_words, int *bad_index, void *stream);

#ifdef __cplusplus
}
#endif
#endif
