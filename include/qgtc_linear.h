/* qgtc_linear.h — the byte-code route of the affine linear layer on libqgtc_hip.so: out ~ X W with X [M, K]
 * quantised per tensor and W [K, N] per output column (or per tensor), the product of the codes on the int8 matrix instruction
 * (v_mfma_i32_16x16x64_i8) with an int32 accumulator, and the dequantising epilogue of qgtc_affine_dequant in the same launch. X's codes
 * never reach memory: the launch reads float32 X, quantises it in registers and feeds the instruction. The quantise rule, the qparams
 * rows and the accumulator identity are those of qgtc_affine.h. The ABI version of qgtc.h does not change: these are entries added
 * beside it. tests/affine_model.py states every bit of what follows in NumPy.
 *
 * TRANSPOSED WEIGHT CODES: uint8 [N, ldk], code (k, n) of W at byte n * ldk + k, so that the K codes of an output column are contiguous
 * (the 16-byte right-hand fragments of the instruction). ldk >= K, ldk % 16 == 0 and a 16-byte aligned base (a breach of any of the three
 * is QGTC_EALIGN); the buffer holds at least N * ldk bytes. qgtc_affine_pack_weight writes bytes K .. ldk - 1 of every line as 0;
 * qgtc_affine_linear_u8 accepts anything there.
 *
 * The codes are unsigned, 0 .. 255, and the instruction is signed: inside the launch both sides are shifted by 128 (a' = a - 128,
 * w' = w - 128: one XOR with 0x80 a byte), and the identity of qgtc_affine.h is applied to the shifted codes, zero points and sums -
 *   sum_k (a - za)(w - zb) = acc' - (zb - 128) rs' - (za - 128) cs' + K (za - 128)(zb - 128),     rs' = sum_k a', cs' = col_sums - 128 K
 * - in 64-bit integers, so nothing of the shift shows outside. |a' w'| <= 2^14, hence |acc'| <= K 2^14, and K <= QGTC_LINEAR_K_MAX =
 * 131 071 = 2^17 - 1 keeps it below 2^31; a larger K is refused. There is no 2^24 limit: the accumulator is an integer.
 *
 * Both entries make one launch on `stream` (the last argument), use no atomics, read nothing back and allocate nothing: capturable.
 * Every output word is written. Refusals come before any device work, in this order: QGTC_EINVAL (a NULL required pointer, a dimension
 * < 1, nbits outside 1 .. 8, groups other than 1 or N, K above QGTC_LINEAR_K_MAX), then QGTC_EALIGN (the weight codes off their three
 * rules; a qparams table off a 16-byte boundary; a float32 or int32 buffer off a 4-byte boundary), then QGTC_ESIZE (a buffer too small). */
#ifndef QGTC_LINEAR_H
#define QGTC_LINEAR_H

#include "qgtc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QGTC_LINEAR_K_MAX 131071

/* Weight preparation, one launch on w [K, N] (float32, contiguous, 4-byte aligned): per output column (per_column != 0: N groups) or per
 * tensor (1 group), the range of the group and its qparams row by the rule of qgtc_affine_qparams - bit for bit the rows that entry
 * writes, a min / max being exact in any order -, the codes of the column under the quantise rule of qgtc_affine.h, transposed into
 * codes_t (layout above, pad bytes written 0), and col_sums[n] (int32 [N]) = the sum of column n's codes.
 * qparams_elems >= 4 * groups, codes_bytes >= N * ldk, sums_elems >= N. */
int qgtc_affine_pack_weight(const float *w, int K, int N, int nbits, int per_column, float *qparams, size_t qparams_elems, uint8_t *codes_t,
                            size_t ldk, size_t codes_bytes, int32_t *col_sums, size_t sums_elems, void *stream);

/* The fused product, one launch: out [M, N] (float32, contiguous; out_elems >= M * N) =
 *   t = sum_k (qa_code(x[m][k]) - za)(codes_t[n][k] - zb[n]), exact;   out[m][n] = (float) t * (sa * sb[n]);
 *   then out *= row_scale[m] when given, out += bias[n] when given, out = out > 0 ? out : +0 when relu
 * - one conversion (round to nearest even) and IEEE single operations, one rounding each, never fused: the contract of
 * qgtc_affine_dequant, and bit for bit its result on the float accumulator of the bit-plane product wherever that one is exact.
 * x: float32 [M, K], contiguous, 4-byte aligned (a 16-byte aligned base with K % 4 == 0 is read 16 bytes at a time). qa: the qparams row
 * of x (per tensor; a_bits its width: a NaN product quantises to the zero point, as everywhere). codes_t, ldk, codes_bytes: W's
 * transposed codes. qb: groups_b = 1 or N rows; col_sums: int32 [N]; row_scale (float32 [M]) and bias (float32 [N]) may be NULL. */
int qgtc_affine_linear_u8(const float *x, int M, int K, const float *qa, int a_bits, const uint8_t *codes_t, size_t ldk, size_t codes_bytes,
                          int N, const float *qb, int groups_b, const int32_t *col_sums, const float *row_scale, const float *bias,
                          int relu, float *out, size_t out_elems, void *stream);

#ifdef __cplusplus
}
#endif

#endif
