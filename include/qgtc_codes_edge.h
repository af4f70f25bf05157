/* qgtc_codes_edge.h — the edge-weighted neighbour sum on byte codes on libqgtc_hip.so: the sum every
 * attention layer ends in - one float32 weight per stored cell of the tile-compressed adjacency, and per head - taken on a uint8 code
 * matrix, on both views and under node masks. The code matrix, PAD4, the adjacency, the views and the masks are those of qgtc_codes.h,
 * THE CODE OUTPUT that of qgtc_chain.h, the value index (val_ptr, val_row) and SLOT ORDER those of qgtc.h, "Edge values": tile, then
 * tile row, then column ascending - one array for both views. The ABI version of qgtc.h does not change: these are entries added
 * beside it.
 *
 * Per output row o of the view, with k over the live neighbours of o (a neighbour outside nbr_mask is never loaded, an id >= n is
 * dropped), s(o, k) the slot of the stored cell between them and h = c / (N / heads) the head of column c:
 *   S[o][c] = sum_k values[s(o, k) * heads + h] * ((float) Q[k][c] - z)
 *   y[o][c] = scale * S[o][c]   (* row_scale[o] when row_scale is not NULL)
 * with (scale, z) = row 0 of `qparams` (float32 [1][4], 16-byte aligned, per tensor). `values` is float32 [n_values][heads]; a slot
 * outside [0, n_values) counts as the weight 0. A masked-out cell keeps its slot: the masks change which terms are summed, never which
 * weight a term takes. A row outside row_mask, in a dead block (32 rows on the row view, a k-quad's 128 on the column view: no index
 * and no tile of it is read) or without a live neighbour gives +0; so does any sum that comes out as zero.
 *
 * THERE IS NO ADD-ORDER CONTRACT. The sum is taken in float32, in an order the kernel chooses, with fused multiply-adds; sum w q and
 * sum w are accumulated apart and S = fma(-z, sum w, sum w q). With T_o live terms in row o every element is within
 *   (T_o + 4) * 2^-23 * scale * |row_scale[o]| * (255 + z) * sum_k |w|
 * of the exact value. Where every partial sum is exactly representable (say weights in eighths and sums below 2^24 eighths) the result
 * is exact.
 *
 * With heads > 1 a head's d = N / heads columns must be a multiple of 4 (a lane's four adjacent columns then share a head); other shapes
 * are served on float32 features by qgtc_tiledmm_f32_edge_heads of qgtc_heads.h.
 *
 * The result is stored as exactly one of
 *   out   float32 [n, N], contiguous (out_elems >= n * N);
 *   outq  a code matrix [n, N] (ldo, outq_bytes) under (out_qp, out_bits): THE CODE OUTPUT of qgtc_chain.h applied to y, bit for bit
 *         qgtc_affine_codes of the float result; bytes N .. PAD4(N) - 1 of every row are written 0, bytes from PAD4(N) up to ldo are
 *         left alone. A row that gives +0 comes back as the zero point of out_qp.
 * The destination not given is NULL; its sizes are ignored.
 *
 * Each entry makes one launch on `stream` (the last argument), uses no atomics, reads nothing back and allocates nothing: capturable.
 * Refusals come before any device work, in this order: QGTC_EINVAL (a NULL required pointer - values, val_ptr and val_row are required
 * when n_tiles > 0 -, a dimension < 1, heads < 1, N % heads != 0, heads > 1 with (N / heads) % 4 != 0, n_values > 2^31 - 1, a malformed
 * adjacency, not exactly one output, out_bits outside 1 .. 8 with outq), then QGTC_EALIGN (a code matrix off its three rules; qparams,
 * out_qp, tiles or a mask off a 16-byte boundary; val_ptr off an 8-byte, val_row off a 2-byte, values, row_scale or out off a 4-byte
 * boundary), then QGTC_ESIZE (a buffer too small; mask_words < S128(n) * 4 when a mask is given). An adjacency without tiles
 * (n_tiles == 0) may come with NULL index, tile and value pointers. */
#ifndef QGTC_CODES_EDGE_H
#define QGTC_CODES_EDGE_H

#include "qgtc_codes.h"

#ifdef __cplusplus
extern "C" {
#endif

int qgtc_tiledmm_u8_edge(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const uint8_t *Q, size_t ld,
                         size_t q_bytes, int N, const float *qparams, const float *row_scale, const int64_t *val_ptr, const int16_t *val_row,
                         const float *values, size_t n_values, int heads, float *out, size_t out_elems, uint8_t *outq, size_t ldo,
                         size_t outq_bytes, const float *out_qp, int out_bits, const uint32_t *row_mask, const uint32_t *nbr_mask,
                         size_t mask_words, void *stream);
int qgtc_tiledmm_u8_t_edge(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles, int64_t n_tiles, int n,
                           const uint8_t *Q, size_t ld, size_t q_bytes, int N, const float *qparams, const float *row_scale,
                           const int64_t *val_ptr, const int16_t *val_row, const float *values, size_t n_values, int heads, float *out,
                           size_t out_elems, uint8_t *outq, size_t ldo, size_t outq_bytes, const float *out_qp, int out_bits,
                           const uint32_t *row_mask, const uint32_t *nbr_mask, size_t mask_words, void *stream);

#ifdef __cplusplus
}
#endif

#endif
