/* qgtc_affine.h — uniform affine quantisation on libqgtc_hip.so: x ~ scale * (q - zero_point), from the range of
 * the data, packed into the layouts the bit products already read, and the epilogue that turns their integer accumulators back into real
 * units. The layouts are those of qgtc_val2bit(x, H, W, nbits, col_major, 0, ...) in qgtc.h. The ABI version of qgtc.h does not change:
 * these are entries added beside it. tests/affine_model.py states every bit of what follows in NumPy.
 *
 * All arithmetic is IEEE float32, one rounding per operation named (no fused multiply-add), unless stated. qmax = 2^nbits - 1, nbits
 * 1 .. 8. A GROUP is the whole tensor (groups = 1) or one column of an [H, W] matrix (groups = W).
 *
 * qparams: float32 [groups][4], one row (scale, zero_point, inv_scale, 0) per group.
 *   lo = min(0, min of the group's finite elements), hi = max(0, max of them); NaN and +-inf are ignored; no finite element: lo = hi = 0.
 *   scale = (hi - lo) / qmax, the division correctly rounded; scale < 2^-100 becomes 1 when hi == lo and 2^-100 otherwise.
 *   inv_scale = 1 / scale, correctly rounded.
 *   zero_point = min(max(rint((-lo) * inv_scale), +0), qmax): an integer value kept as a float; rint rounds half to even.
 *
 * quantise: y = x * inv_scale; q = (int) min(max(rint(y) + zero_point, 0), qmax); a NaN y gives zero_point (x NaN), +inf gives qmax, -inf 0.
 *
 * The accumulator identity the epilogue applies: with xa ~ sa (qa - za) over K terms and xb ~ sb[n] (qb - zb[n]),
 *   sum_k (qa[m][k] - za)(qb[k][n] - zb[n]) = acc[m][n] - zb[n] row_sums[m] - za col_sums[n] + K za zb[n]        (exact, int64)
 * where acc is the product of the codes (qgtc_bitmm2int, qgtc_tiledmm2int: float32 holding integers below 2^24), row_sums[m] the sum of
 * qa's row m and col_sums[n] the sum of qb's column n.
 *
 * Every entry checks its arguments before any device work - QGTC_EINVAL (a NULL required pointer, a dimension < 1, nbits outside 1 .. 8,
 * groups other than 1 or the column count), then QGTC_EALIGN (a packed pointer or a qparams table off a 16-byte boundary), then QGTC_ESIZE
 * (a buffer too small) -, takes the stream last, enqueues on it and returns. No atomics, no host read, no allocation: capturable. */
#ifndef QGTC_AFFINE_H
#define QGTC_AFFINE_H

#include "qgtc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 32-bit words of scratch qgtc_affine_qparams needs for an [H, W] input (0 for a non-positive dimension). Never cleared by the caller. */
size_t qgtc_affine_work_words(int H, int W, int per_column);

/* The range launch: qparams [groups][4] of x [H, W] (groups = W with per_column, else 1; qparams_elems >= 4 * groups; 16-byte aligned).
 * Two launches: every workgroup writes the (lo, hi) of its share into `work`, a finishing launch folds them and computes the four floats of
 * every group. Each word of `work` that is read has been written by the first launch, and every element of qparams is written. Per column,
 * a wave reads 64 adjacent columns of one row at a time. */
int qgtc_affine_qparams(const float *x, int H, int W, int nbits, int per_column, float *qparams, size_t qparams_elems, uint32_t *work,
                        size_t work_words, void *stream);

/* Quantise x [H, W] with the rows of `qparams` (groups = 1: row 0 for every element; groups = W: row c for column c) and pack the codes:
 * out holds the words of qgtc_val2bit(.., col_major, output_layer = 0) of a matrix of those codes - rows layout [nbits][PAD8(H)][S128(W)*4],
 * cols layout [nbits][PAD128(W)][S128(H)*4]; element i of a line at word i >> 5, bit 31 - (i & 31); every pad word and pad bit written (0).
 * One read of x. sums (int32, or NULL): rows layout [H], sums[r] = the sum of row r's codes; cols layout [W], sums[c] = the sum of
 * column c's codes - from a second, small launch that counts the bits of the packed planes (exact, the same on every launch).
 * out and qparams 16-byte aligned; x needs 4-byte alignment only. */
int qgtc_val2bit_affine(const float *x, int H, int W, int nbits, int col_major, const float *qparams, int groups, uint32_t *out,
                        size_t out_words, int32_t *sums, size_t sums_elems, void *stream);

/* The dequantising epilogue on acc [M, N] (float32 holding integers):
 *   t = (int64) acc[m][n] - zb[n] row_sums[m] - za col_sums[n] + K za zb[n];   out[m][n] = (float) t * (sa * sb[n]);
 *   then out *= row_scale[m] when given, out += bias[n] when given, out = out > 0 ? out : +0 when relu.
 * qa: one row of qparams (the left operand, per tensor); qb: groups_b = 1 or N rows. A NULL row_sums leaves zb row_sums out (the caller
 * asserts it is zero), a NULL col_sums likewise za col_sums. out may be acc itself. out_elems >= M * N; qa and qb 16-byte aligned. */
int qgtc_affine_dequant(const float *acc, int M, int N, int K, const float *qa, const int32_t *row_sums, const float *qb, int groups_b,
                        const int32_t *col_sums, const float *row_scale, const float *bias, int relu, float *out, size_t out_elems,
                        void *stream);

#ifdef __cplusplus
}
#endif

#endif
