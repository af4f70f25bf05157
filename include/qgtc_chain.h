/* qgtc_chain.h — the static affine chain on libqgtc_hip.so: the byte-code product of qgtc_linear.h and the
 * byte-code walks of qgtc_codes.h with uint8 codes on either side of the launch, under quantisation parameters the caller fixes
 * (calibrated once) instead of a range taken from the data. A producer re-quantises in its epilogue, so an activation crosses memory
 * once, one byte an element, and a layer float -> codes -> codes -> codes -> float is one launch a stage. The quantise rule and the
 * qparams rows are those of qgtc_affine.h, the weight operand and QGTC_LINEAR_K_MAX those of qgtc_linear.h, the adjacency, the masks and
 * the walks those of qgtc_codes.h. The ABI version of qgtc.h does not change: these are entries added beside it.
 *
 * A CODE MATRIX (input or output) is that of qgtc_codes.h: uint8 [rows, ld], code (r, c) at byte r * ld + c, ld >= cols, ld % 4 == 0 and
 * a 4-byte aligned base (a breach of any of the three is QGTC_EALIGN); the buffer holds at least (rows - 1) * ld + PAD4(cols) bytes. A
 * consumer accepts anything in bytes cols .. ld - 1 of a row. A producer writes bytes cols .. PAD4(cols) - 1 of every row as 0 and leaves
 * bytes from PAD4(cols) on untouched. Input codes are taken as they are, 0 .. 255, never clamped to a bit width.
 *
 * THE CODE OUTPUT of every entry: the float `o` its float-producing twin would have stored, every rounding included, then
 *   y = o * inv;   code = y != y ? zp : min(max(rint(y) + zp, 0), 2^out_bits - 1)           (scale, zp, inv, 0) = row 0 of out_qp
 * - the quantise rule of qgtc_affine.h under one per-tensor row out_qp (float32 [1][4], 16-byte aligned): bit for bit qgtc_affine_codes
 * applied to the twin's output.
 *
 * Every entry makes one launch on `stream` (the last argument), uses no atomics, reads nothing back and allocates nothing: capturable.
 * Every output byte an entry owns is written. Refusals come before any device work, in this order: QGTC_EINVAL (a NULL required
 * pointer, a dimension < 1, a bit width outside 1 .. 8, groups other than 1 or N, K above QGTC_LINEAR_K_MAX, a malformed adjacency, not
 * exactly one left operand or not exactly one output, float in with float out), then QGTC_EALIGN (a code matrix or the weight codes off
 * their rules; a qparams table, tiles or a mask off a 16-byte boundary; a float32 or int32 buffer off a 4-byte boundary), then
 * QGTC_ESIZE (a buffer too small; mask_words < S128(n) * 4 when a mask is given). */
#ifndef QGTC_CHAIN_H
#define QGTC_CHAIN_H

#include "qgtc_linear.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The chain product, one launch: the product of qgtc_affine_linear_u8 -
 *   t = sum_k (a[m][k] - za)(codes_t[n][k] - zb[n]), exact;   o = (float) t * (sa * sb[n]);   o *= row_scale[m];  o += bias[n];  relu
 * - with the left operand given as exactly one of
 *   x   float32 [M, K], contiguous, 4-byte aligned: a = its code under (qa, a_bits), quantised in registers as qgtc_affine_linear_u8 does;
 *   xq  a code matrix [M, K] (ldx, xq_bytes): a = the byte itself (qa is its row; a_bits is validated and otherwise unused)
 * and the result stored as exactly one of
 *   out   float32 [M, N], contiguous (out_elems >= M * N): bit for bit the store of qgtc_affine_linear_u8;
 *   outq  a code matrix [M, N] (ldo, outq_bytes) under (out_qp, out_bits): THE CODE OUTPUT above.
 * The operand not given is NULL; its sizes are ignored. x with out is qgtc_affine_linear_u8 itself and is refused here (QGTC_EINVAL).
 * codes_t, ldk, codes_bytes, qb, groups_b, col_sums, row_scale, bias, relu: as in qgtc_linear.h. */
int qgtc_affine_linear_chain(const float *x, const uint8_t *xq, size_t ldx, size_t xq_bytes, int M, int K, const float *qa, int a_bits,
                             const uint8_t *codes_t, size_t ldk, size_t codes_bytes, int N, const float *qb, int groups_b,
                             const int32_t *col_sums, const float *row_scale, const float *bias, int relu, float *out, size_t out_elems,
                             uint8_t *outq, size_t ldo, size_t outq_bytes, const float *out_qp, int out_bits, void *stream);

/* The walks of qgtc_tiledmm_u8_affine / qgtc_tiledmm_u8_t_affine with THE CODE OUTPUT: per element the float of those entries
 * (t = acc - z * cnt in 64 bits, one conversion, * scale, * row_scale[o] when given), then the quantise rule under (out_qp, out_bits)
 * into the code matrix outq [n, N] (ldo, outq_bytes). A row outside row_mask, in a dead block or without live neighbours is float +0 and
 * so comes back as the code zp of out_qp, not 0. */
int qgtc_tiledmm_u8_requant(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const uint8_t *Q,
                            size_t ld, size_t q_bytes, int N, const float *qparams, const float *row_scale, const float *out_qp,
                            int out_bits, uint8_t *outq, size_t ldo, size_t outq_bytes, const uint32_t *row_mask, const uint32_t *nbr_mask,
                            size_t mask_words, void *stream);
int qgtc_tiledmm_u8_t_requant(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles, int64_t n_tiles,
                              int n, const uint8_t *Q, size_t ld, size_t q_bytes, int N, const float *qparams, const float *row_scale,
                              const float *out_qp, int out_bits, uint8_t *outq, size_t ldo, size_t outq_bytes, const uint32_t *row_mask,
                              const uint32_t *nbr_mask, size_t mask_words, void *stream);

#ifdef __cplusplus
}
#endif

#endif
