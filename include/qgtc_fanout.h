/* qgtc_fanout.h — fixed-fanout neighbour sampling on the tiled adjacency of libqgtc_hip.so (GraphSAGE, Hamilton et al. 2017; DESIGN.md
 * section 6.15l): at most k neighbours per node, decided inside the tile walk, so that no second adjacency is built. The terms - view,
 * output row, neighbour, the cell (i, j) of A in the adjacency's own numbering on BOTH views - and the hash H(i, j, seed) are those of
 * "Edge dropout" in qgtc.h. The ABI version of qgtc.h does not change: these are entries added beside it, declared in a header of their own.
 *
 * The rule. A sample of fanout k >= 1 with a 64-bit seed is taken on one AXIS: the rows of A (sampled on the row view) or the columns
 * of A (sampled on the column view, the _t entries). For a node u of that axis let deg be the number of its set cells whose other
 * coordinate is < n (the cells of row u, or of column u):
 *     thr[u] = 0                                                    if deg <= k
 *     thr[u] = the k-th largest of H(i, j, seed) over those cells   otherwise
 * and cell (i, j) is KEPT when H(i, j, seed) >= thr[u], with u = i on the row axis and u = j on the column axis. thr is uint32 [n].
 *
 * mix32 is a bijection on uint32 (xorshifts and odd multiplies are invertible), so for fixed i and seed the map j -> H(i, j, seed) is
 * a bijection, and likewise i -> H(i, j, seed) for fixed j: the hashes of one row's cells, or of one column's, are pairwise distinct
 * and the k-th largest is unique. Consequences:
 *   - exactly min(deg, k) cells are kept per node of the axis, never more;
 *   - k >= deg keeps every cell of the node (thr = 0), so k >= the largest degree gives the unsampled operators' bits;
 *   - under one seed the sample for k is a subset of the sample for k + 1 (the threshold does not rise with k);
 *   - keeping the k largest of distinct pseudo-random keys is a draw without replacement; a row-axis sample and a column-axis sample of
 *     one seed are different samples (each bounds the degree on its own axis only).
 *
 * Selection. qgtc_tiled_fanout_thr computes thr on the row axis, qgtc_tiled_fanout_thr_t on the column axis: one launch on `stream`, no
 * atomics, no host read, every element thr[0 .. n) written with a plain store and nothing past them. One wavefront owns one node: it
 * counts the node's cells, stores 0 when there are at most k, and otherwise finds the k-th largest hash exactly, MSB first in 32
 * counting steps - over the node's hashes held in LDS when there are at most 1024 of them, by walking the node's tiles again when there
 * are more. No degree is too large. The result is a function of (adjacency, n, k, seed) alone. Tiles whose k-quad or row block lies
 * outside the matrix are skipped, as the products skip them. n_tiles == 0 with NULL index pointers is an adjacency without edges: all
 * thr are 0.
 * Refusals, before any device work, in the order invalid, alignment, size: QGTC_EINVAL for a NULL thr, k < 1, n outside 1 .. 2^23,
 * n_tiles < 0 and a missing index or tile array when n_tiles > 0; QGTC_EALIGN for tiles off a 16-byte and thr off a 4-byte boundary;
 * QGTC_ESIZE for thr_elems < n.
 *
 * The mask in the tile walk. Each _fanout entry is its _drop twin of qgtc.h with (thr, thr_of_nbr, seed) in place of (threshold, seed):
 *   thr_of_nbr = 0 (own): thr belongs to the OUTPUT rows of the launch - a sample taken on the view the entry walks. Output row o keeps
 *                neighbour v when H(cell) >= thr[o]: the _drop kernel's code with the row's own threshold.
 *   thr_of_nbr = 1 (nbr): thr belongs to the NEIGHBOURS - a sample taken on the other view, which is what every backward uses. Output row
 *                o keeps neighbour v when H(cell) >= thr[v]; thr[v] is loaded as the set bit is decoded.
 * Masking is dropping, as for edge dropout: each entry returns bit for bit what its unmasked parent returns on an adjacency packed from
 * the kept cells only; a dropped neighbour's row is never loaded; nothing is rescaled (the mean over a sample takes
 * row_scale = 1 / min(deg, k)). In the attention forward `shift` must be the maximum over the KEPT neighbours (qgtc_tiledmax_f32_fanout
 * / _t_fanout with N = 1 and the same sample). thr must hold n elements; it is read on the device, so a captured graph follows its
 * contents. Each entry keeps its _drop twin's refusals in that order, plus QGTC_EINVAL for a NULL thr and for thr_of_nbr outside {0, 1}
 * (with the other invalid arguments, before any alignment refusal) and QGTC_EALIGN for thr off a 4-byte boundary. */
#ifndef QGTC_FANOUT_H
#define QGTC_FANOUT_H

#include "qgtc.h"

#ifdef __cplusplus
extern "C" {
#endif

int qgtc_tiled_fanout_thr(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, int k,
                          uint64_t seed, uint32_t *thr, size_t thr_elems, void *stream);
int qgtc_tiled_fanout_thr_t(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                            int64_t n_tiles, int n, int k, uint64_t seed, uint32_t *thr, size_t thr_elems, void *stream);

int qgtc_tiledmm_f32_fanout(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *X,
                            size_t x_elems, int N, const float *row_scale, const float *src_scale, float *out, size_t out_elems,
                            const uint32_t *thr, int thr_of_nbr, uint64_t seed, void *stream);
int qgtc_tiledmm_f32_t_fanout(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                              int64_t n_tiles, int n, const float *X, size_t x_elems, int N, const float *row_scale,
                              const float *src_scale, float *out, size_t out_elems, const uint32_t *thr, int thr_of_nbr, uint64_t seed,
                              void *stream);
int qgtc_tiledmax_f32_fanout(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *X,
                             size_t x_elems, int N, int op, float *out, size_t out_elems, int32_t *arg, size_t arg_elems,
                             const uint32_t *thr, int thr_of_nbr, uint64_t seed, void *stream);
int qgtc_tiledmax_f32_t_fanout(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                               int64_t n_tiles, int n, const float *X, size_t x_elems, int N, int op, float *out, size_t out_elems,
                               int32_t *arg, size_t arg_elems, const uint32_t *thr, int thr_of_nbr, uint64_t seed, void *stream);
int qgtc_tiledatt_f32_fanout(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *X,
                             size_t x_elems, int N, const float *att_own, const float *att_nbr, float negative_slope, int backward,
                             const float *shift, float *m, float *inv, float *out, size_t out_elems, const uint32_t *thr, int thr_of_nbr,
                             uint64_t seed, void *stream);
int qgtc_tiledatt_f32_t_fanout(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                               int64_t n_tiles, int n, const float *X, size_t x_elems, int N, const float *att_own, const float *att_nbr,
                               float negative_slope, int backward, const float *shift, float *m, float *inv, float *out,
                               size_t out_elems, const uint32_t *thr, int thr_of_nbr, uint64_t seed, void *stream);
int qgtc_tiledatt_grad_f32_fanout(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n,
                                  const float *A, const float *B, size_t ab_elems, int N, const float *att_own, const float *att_nbr,
                                  float negative_slope, int nbr_owns, const float *m, const float *inv, const float *D, float *out,
                                  size_t out_elems, const uint32_t *thr, int thr_of_nbr, uint64_t seed, void *stream);
int qgtc_tiledatt_grad_f32_t_fanout(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                                    int64_t n_tiles, int n, const float *A, const float *B, size_t ab_elems, int N, const float *att_own,
                                    const float *att_nbr, float negative_slope, int nbr_owns, const float *m, const float *inv,
                                    const float *D, float *out, size_t out_elems, const uint32_t *thr, int thr_of_nbr, uint64_t seed,
                                    void *stream);

#ifdef __cplusplus
}
#endif

#endif
