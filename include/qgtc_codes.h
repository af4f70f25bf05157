/* qgtc_codes.h — the byte-code route of affine quantisation on libqgtc_hip.so: the codes of qgtc_affine.h kept
 * one byte each instead of as bit planes, and the neighbour sum of such codes on the tile-compressed adjacency as a gather - a tile is
 * read as a compressed neighbour list, as the float products read it, and one dword of four codes is loaded per neighbour and lane - with
 * the dequantising epilogue of qgtc_affine_dequant in the same launch. The terms view, k-quad and tile are those of "Tile-compressed
 * adjacency" and "Transposed tiled adjacency" in qgtc.h, the masks those of "Node masks" there and of qgtc_bitnodes.h, the quantise rule
 * and qparams those of qgtc_affine.h. The ABI version of qgtc.h does not change: these are entries added beside it.
 * tests/tiled_codes_model.py states every bit of what follows in NumPy.
 *
 * A CODE MATRIX is uint8 [H, W] with a row stride `ld` in bytes: code (r, c) at byte r * ld + c. ld >= W, ld % 4 == 0 and a 4-byte aligned
 * base (a breach of any of the three is QGTC_EALIGN), so that the four codes of columns 4 j .. 4 j + 3 of a row are one aligned dword.
 * PAD4(W) = (W + 3) / 4 * 4. The buffer holds at least (H - 1) * ld + PAD4(W) bytes. As an input, the bytes of a row from column W up to ld
 * may hold anything: a dword that straddles W is loaded whole and its surplus bytes are dropped.
 *
 * Integer sums are exact in any order, so nothing here has an add-order contract. A sum is int32: degree * 255 < 2^31 for every n the
 * tiled adjacency admits (n <= 2^23).
 *
 * Every entry makes one launch on `stream` (the last argument), uses no atomics, reads nothing back and allocates nothing: capturable.
 * Refusals come before any device work, in this order: QGTC_EINVAL (a NULL required pointer, a dimension < 1, nbits outside 1 .. 8,
 * groups other than 1 or W, a malformed adjacency), then QGTC_EALIGN (a code matrix off its three rules; qparams, tiles or a mask off a
 * 16-byte boundary; an int32 or float32 buffer off a 4-byte boundary), then QGTC_ESIZE (a buffer too small; mask_words < S128(n) * 4 when a
 * mask is given). An adjacency without tiles (n_tiles == 0) may come with NULL index and tile pointers. */
#ifndef QGTC_CODES_H
#define QGTC_CODES_H

#include "qgtc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out[r * ld + c] = the code of x[r][c] under the quantise rule of qgtc_affine.h (NaN, +-inf and the clamp included) with the rows of
 * `qparams` (groups = 1: row 0 for every element; groups = W: row c for column c; 16-byte aligned). Bytes W .. PAD4(W) - 1 of every row
 * are written 0, bytes from PAD4(W) up to ld are left alone. One read of x; x needs 4-byte alignment only. */
int qgtc_affine_codes(const float *x, int H, int W, int nbits, const float *qparams, int groups, uint8_t *out, size_t ld, size_t out_bytes,
                      void *stream);

/* out (int32 [n, N], contiguous; out_elems >= n * N) [o][c] = the exact sum of Q[k][c] over the live neighbours k of output row o on the
 * view: Q is a code matrix [n, N] (ld, q_bytes) in the adjacency's numbering. row_mask / nbr_mask are bitmaps or NULL (all nodes),
 * relative to the view the entry walks; mask_words is the length of each bitmap given. A row outside row_mask gives 0; a neighbour outside
 * nbr_mask is never loaded; a block without a live row (32 rows on the row view, a k-quad's 128 on the column view) reads no index and no
 * tile; a neighbour id >= n is dropped. So the tiles of a dead block and the code bytes of dead neighbours may hold anything. Every one of
 * the n * N outputs is written. */
int qgtc_tiledmm_u8(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const uint8_t *Q, size_t ld,
                    size_t q_bytes, int N, int32_t *out, size_t out_elems, const uint32_t *row_mask, const uint32_t *nbr_mask,
                    size_t mask_words, void *stream);
int qgtc_tiledmm_u8_t(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles, int64_t n_tiles, int n,
                      const uint8_t *Q, size_t ld, size_t q_bytes, int N, int32_t *out, size_t out_elems, const uint32_t *row_mask,
                      const uint32_t *nbr_mask, size_t mask_words, void *stream);

/* The same walk, then the dequantising epilogue on every row o, computed or not (out float32 [n, N]):
 *   t = (int64) acc[o][c] - (int64) z * cnt[o];   y = (float) t * scale;   y = y * row_scale[o] when row_scale is given
 * - one conversion (round to nearest even) and one IEEE single multiply each, never fused. (scale, z) = row 0 of `qparams` (float32 [1][4],
 * 16-byte aligned, per tensor); cnt[o] = the number of terms added into row o, counted by the walk: the degree under the masks. A row
 * outside row_mask or in a dead block has acc = cnt = 0. Bit for bit qgtc_affine_dequant(acc, n, N, n, (1, 0, 1, 0), cnt, qparams, 1, NULL,
 * row_scale, NULL, 0, ..) on the sums of the entry above. row_scale: float32 [n] or NULL. */
int qgtc_tiledmm_u8_affine(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const uint8_t *Q,
                           size_t ld, size_t q_bytes, int N, const float *qparams, const float *row_scale, float *out, size_t out_elems,
                           const uint32_t *row_mask, const uint32_t *nbr_mask, size_t mask_words, void *stream);
int qgtc_tiledmm_u8_t_affine(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles, int64_t n_tiles,
                             int n, const uint8_t *Q, size_t ld, size_t q_bytes, int N, const float *qparams, const float *row_scale,
                             float *out, size_t out_elems, const uint32_t *row_mask, const uint32_t *nbr_mask, size_t mask_words,
                             void *stream);

#ifdef __cplusplus
}
#endif

#endif
