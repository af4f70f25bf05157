/* qgtc_blocks.h — mini-batch GraphSAGE on the tiled adjacency of libqgtc_hip.so: a fixed-fanout sample of an
 * INDUCED SUBGRAPH, its frontier as a node bitmap, and the sampled aggregates under that sample. The terms view, axis, cell, H(i, j, seed)
 * and the own / nbr form are those of qgtc_fanout.h; a bitmap is that of "Node masks" in qgtc.h (node i at word i >> 5, bit 31 - (i & 31),
 * S128(n) * 4 words, 16-byte aligned). The ABI version of qgtc.h does not change: these are entries added beside it.
 *
 * The masked sample is taken on a view under a row_mask and a nbr_mask, each a bitmap relative to THAT view or NULL (all nodes); mask_words
 * is the length of each bitmap given. For a node u of row_mask, deg_m(u) is the number of its set cells whose other end is < n and in
 * nbr_mask:
 *     thr[u] = 0 if deg_m(u) <= k, otherwise the k-th largest of H over exactly those cells;   kept[u] = min(deg_m(u), k)
 * and for u outside row_mask thr[u] = 0, kept[u] = 0 and none of u's tiles is read. Ids do not change under masking: the sample is, word
 * for word, qgtc_tiled_fanout_thr / _t on the adjacency packed from the edges with the row end in row_mask and the neighbour end in
 * nbr_mask.
 *
 * Selection. qgtc_tiled_fanout_thr_nodes (row axis) and qgtc_tiled_fanout_thr_t_nodes (column axis) are the selection launches of
 * qgtc_fanout.h with the masks and an optional kept (int32 [n]; NULL: not wanted): one launch on `stream`, no atomics, no host read, every
 * thr[0 .. n) and kept[0 .. n) written with a plain store. The path is chosen by deg_m, not by the unmasked degree. Two NULL masks give
 * qgtc_tiled_fanout_thr's words. Refusals before any device work: those of qgtc_tiled_fanout_thr in its order, with kept off a 4-byte
 * boundary among the QGTC_EALIGN causes and kept_elems < n (kept given) among the QGTC_ESIZE causes; then those of the node masks
 * (QGTC_ESIZE for mask_words < S128(n) * 4 when a mask is given, QGTC_EALIGN for a mask off a 16-byte boundary).
 *
 * Frontier. out[S128(n) * 4] is the bitmap of the nodes the kept cells reach: bit v is set iff some cell joins a node u of row_mask to
 * neighbour v of nbr_mask with H >= thr[u], or v is in `include` (a bitmap or NULL; normally row_mask, so that a layer's inputs contain
 * its outputs). Bits from n up and pad words are 0, whatever include holds there. One launch, no atomics and no clear: every word of
 * out is written exactly once with a plain store. The output is indexed by the NEIGHBOUR, so each entry takes the index of the OTHER view:
 *   qgtc_tiled_fanout_frontier    a row-axis sample (thr of qgtc_tiled_fanout_thr_nodes); takes the column index. One workgroup per k-quad.
 *   qgtc_tiled_fanout_frontier_t  a column-axis sample (thr of _thr_t_nodes); takes the row index. One workgroup per word of out.
 * The masks are the sample's, relative to the sample's view. n_tiles == 0 with NULL indices is legal: out is include, or 0.
 * Refusals: QGTC_EINVAL for a NULL thr or out and a malformed adjacency; QGTC_EALIGN for tiles, out, include or a mask off a 16-byte and
 * thr off a 4-byte boundary; QGTC_ESIZE for out_words < S128(n) * 4 and for mask_words < S128(n) * 4 when a mask or include is given
 * (include has mask_words words too).
 *
 * Aggregates. Each _fanout_nodes entry is its _fanout twin of qgtc_fanout.h plus (row_mask, nbr_mask, mask_words) of the _nodes entries of
 * qgtc.h, relative to the view the ENTRY walks: on the sample's view pass the sample's masks and thr_of_nbr = 0, on the other view the two
 * masks swapped and thr_of_nbr = 1 - as every backward does with scales and masks. The result is, bit for bit, the plain entry on the
 * adjacency packed from the kept cells; output rows outside row_mask are +0 (the attention's m and inv as in the _nodes entries). The
 * attention forward's `shift` is the maximum over the kept neighbours (qgtc_tiledmax_f32_fanout_nodes / _t with N = 1, the same sample
 * and masks). Refusals: the twin's, in its order, then the node masks'. */
#ifndef QGTC_BLOCKS_H
#define QGTC_BLOCKS_H

#include "qgtc.h"

#ifdef __cplusplus
extern "C" {
#endif

int qgtc_tiled_fanout_thr_nodes(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, int k,
                                uint64_t seed, uint32_t *thr, size_t thr_elems, int32_t *kept, size_t kept_elems,
                                const uint32_t *row_mask, const uint32_t *nbr_mask, size_t mask_words, void *stream);
int qgtc_tiled_fanout_thr_t_nodes(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                                  int64_t n_tiles, int n, int k, uint64_t seed, uint32_t *thr, size_t thr_elems, int32_t *kept,
                                  size_t kept_elems, const uint32_t *row_mask, const uint32_t *nbr_mask, size_t mask_words, void *stream);

int qgtc_tiled_fanout_frontier(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                               int64_t n_tiles, int n, const uint32_t *thr, uint64_t seed, const uint32_t *row_mask,
                               const uint32_t *nbr_mask, const uint32_t *include, size_t mask_words, uint32_t *out, size_t out_words,
                               void *stream);
int qgtc_tiled_fanout_frontier_t(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n,
                                 const uint32_t *thr, uint64_t seed, const uint32_t *row_mask, const uint32_t *nbr_mask,
                                 const uint32_t *include, size_t mask_words, uint32_t *out, size_t out_words, void *stream);

int qgtc_tiledmm_f32_fanout_nodes(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n,
                                  const float *X, size_t x_elems, int N, const float *row_scale, const float *src_scale, float *out,
                                  size_t out_elems, const uint32_t *thr, int thr_of_nbr, uint64_t seed, const uint32_t *row_mask,
                                  const uint32_t *nbr_mask, size_t mask_words, void *stream);
int qgtc_tiledmm_f32_t_fanout_nodes(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                                    int64_t n_tiles, int n, const float *X, size_t x_elems, int N, const float *row_scale,
                                    const float *src_scale, float *out, size_t out_elems, const uint32_t *thr, int thr_of_nbr,
                                    uint64_t seed, const uint32_t *row_mask, const uint32_t *nbr_mask, size_t mask_words, void *stream);
int qgtc_tiledmax_f32_fanout_nodes(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n,
                                   const float *X, size_t x_elems, int N, int op, float *out, size_t out_elems, int32_t *arg,
                                   size_t arg_elems, const uint32_t *thr, int thr_of_nbr, uint64_t seed, const uint32_t *row_mask,
                                   const uint32_t *nbr_mask, size_t mask_words, void *stream);
int qgtc_tiledmax_f32_t_fanout_nodes(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                                     int64_t n_tiles, int n, const float *X, size_t x_elems, int N, int op, float *out, size_t out_elems,
                                     int32_t *arg, size_t arg_elems, const uint32_t *thr, int thr_of_nbr, uint64_t seed,
                                     const uint32_t *row_mask, const uint32_t *nbr_mask, size_t mask_words, void *stream);
int qgtc_tiledatt_f32_fanout_nodes(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n,
                                   const float *X, size_t x_elems, int N, const float *att_own, const float *att_nbr, float negative_slope,
                                   int backward, const float *shift, float *m, float *inv, float *out, size_t out_elems,
                                   const uint32_t *thr, int thr_of_nbr, uint64_t seed, const uint32_t *row_mask, const uint32_t *nbr_mask,
                                   size_t mask_words, void *stream);
int qgtc_tiledatt_f32_t_fanout_nodes(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                                     int64_t n_tiles, int n, const float *X, size_t x_elems, int N, const float *att_own,
                                     const float *att_nbr, float negative_slope, int backward, const float *shift, float *m, float *inv,
                                     float *out, size_t out_elems, const uint32_t *thr, int thr_of_nbr, uint64_t seed,
                                     const uint32_t *row_mask, const uint32_t *nbr_mask, size_t mask_words, void *stream);
int qgtc_tiledatt_grad_f32_fanout_nodes(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n,
                                        const float *A, const float *B, size_t ab_elems, int N, const float *att_own, const float *att_nbr,
                                        float negative_slope, int nbr_owns, const float *m, const float *inv, const float *D, float *out,
                                        size_t out_elems, const uint32_t *thr, int thr_of_nbr, uint64_t seed, const uint32_t *row_mask,
                                        const uint32_t *nbr_mask, size_t mask_words, void *stream);
int qgtc_tiledatt_grad_f32_t_fanout_nodes(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                                          int64_t n_tiles, int n, const float *A, const float *B, size_t ab_elems, int N,
                                          const float *att_own, const float *att_nbr, float negative_slope, int nbr_owns, const float *m,
                                          const float *inv, const float *D, float *out, size_t out_elems, const uint32_t *thr,
                                          int thr_of_nbr, uint64_t seed, const uint32_t *row_mask, const uint32_t *nbr_mask,
                                          size_t mask_words, void *stream);

#ifdef __cplusplus
}
#endif

#endif
