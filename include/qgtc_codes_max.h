/* qgtc_codes_max.h — max and min aggregation on byte codes on libqgtc_hip.so: the element-wise extremum of the
 * neighbours' code rows on the tile-compressed adjacency, on both views and under node masks. The quantise rule of qgtc_affine.h is
 * monotone non-decreasing, so the extremum of the codes is the code of the extremum: the walk's output is itself a code matrix under the
 * operand's own qparams row, with no accumulator growth, no term count and no aggregation error, and it can feed the next product of the
 * static chain (qgtc_chain.h) one byte an element. The code matrix, PAD4, the adjacency, the views and the masks are those of
 * qgtc_codes.h, THE CODE OUTPUT that of qgtc_chain.h. The ABI version of qgtc.h does not change: these are entries added beside it.
 *
 * Per output row o of the view, with k over the live neighbours of o (a neighbour outside nbr_mask is never loaded, an id >= n is dropped):
 *   m[o][c] = max_k Q[k][c]   (is_min == 0)      or      min_k Q[k][c]   (is_min != 0)
 * A row outside row_mask, in a dead block (32 rows on the row view, a k-quad's 128 on the column view: no index and no tile of it is read)
 * or without a live neighbour HAS NO TERM. Bytes are compared as unsigned 0 .. 255, whatever bit width they were made under.
 *
 * Every entry makes one launch on `stream` (the last argument), uses no atomics, reads nothing back and allocates nothing: capturable.
 * Every output an entry owns is written. Refusals come before any device work, in this order: QGTC_EINVAL (a NULL required pointer, a
 * dimension < 1, empty_code outside 0 .. 255, a malformed adjacency, not exactly one output, out_bits outside 1 .. 8 with outq), then
 * QGTC_EALIGN (a code matrix off its three rules; qparams, tiles or a mask off a 16-byte boundary; a float32 buffer off a 4-byte
 * boundary), then QGTC_ESIZE (a buffer too small; mask_words < S128(n) * 4 when a mask is given). An adjacency without tiles
 * (n_tiles == 0) may come with NULL index and tile pointers. */
#ifndef QGTC_CODES_MAX_H
#define QGTC_CODES_MAX_H

#include "qgtc_codes.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out: a code matrix [n, N] (ldo, out_bytes) with out[o][c] = m[o][c], or empty_code in a row that has no term. Bytes N .. PAD4(N) - 1 of
 * every row are written 0, bytes from PAD4(N) up to ldo are left alone. */
int qgtc_tiledmax_u8(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const uint8_t *Q, size_t ld,
                     size_t q_bytes, int N, int is_min, int empty_code, uint8_t *out, size_t ldo, size_t out_bytes, const uint32_t *row_mask,
                     const uint32_t *nbr_mask, size_t mask_words, void *stream);
int qgtc_tiledmax_u8_t(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles, int64_t n_tiles, int n,
                       const uint8_t *Q, size_t ld, size_t q_bytes, int N, int is_min, int empty_code, uint8_t *out, size_t ldo,
                       size_t out_bytes, const uint32_t *row_mask, const uint32_t *nbr_mask, size_t mask_words, void *stream);

/* The same walk with the dequantising epilogue on every row, computed or not:
 *   y = (float) ((int) m[o][c] - z) * scale        (scale, z) = row 0 of `qparams` (float32 [1][4], 16-byte aligned, per tensor)
 * - one integer subtraction, one conversion and one IEEE single multiply, never fused; a row that has no term gives +0. There is no
 * row_scale: an extremum is not scaled. The result is stored as exactly one of
 *   out   float32 [n, N], contiguous (out_elems >= n * N);
 *   outq  a code matrix [n, N] (ldo, outq_bytes) under (out_qp, out_bits): THE CODE OUTPUT of qgtc_chain.h applied to y, bit for bit
 *         qgtc_affine_codes of the float result. A row that has no term is float +0 and so comes back as the zero point of out_qp.
 * The destination not given is NULL; its sizes are ignored. */
int qgtc_tiledmax_u8_affine(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const uint8_t *Q,
                            size_t ld, size_t q_bytes, int N, const float *qparams, int is_min, float *out, size_t out_elems, uint8_t *outq,
                            size_t ldo, size_t outq_bytes, const float *out_qp, int out_bits, const uint32_t *row_mask,
                            const uint32_t *nbr_mask, size_t mask_words, void *stream);
int qgtc_tiledmax_u8_t_affine(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles, int64_t n_tiles,
                              int n, const uint8_t *Q, size_t ld, size_t q_bytes, int N, const float *qparams, int is_min, float *out,
                              size_t out_elems, uint8_t *outq, size_t ldo, size_t outq_bytes, const float *out_qp, int out_bits,
                              const uint32_t *row_mask, const uint32_t *nbr_mask, size_t mask_words, void *stream);

#ifdef __cplusplus
}
#endif

#endif
