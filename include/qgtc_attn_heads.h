/* qgtc_attn_heads.h — the multi-head entries of libqgtc_hip.so's attention path (`attn=(p, q)`, the reducer of GAT): the softmax-weighted
 * sum, its backward product, the two score gradients and the row dot, each for H heads in ONE launch. They
 * generalise thirteen entries of qgtc.h ("Attention tiled products", "Edge dropout", "Node masks"), whose terms - L, EXP, DOT, the
 * shift, the order of every fold, the masks - are used here unchanged. The ABI version of qgtc.h does not change: these are entries
 * added beside it, declared in a header of their own like qgtc_heads.h.
 *
 * Layout. A node matrix (X, dY, A, B, out of the products) is float32 [n, N] with N = H * d and head h in the columns
 * h * d .. (h + 1) * d - 1. Every per-node vector of the single-head entries - att_own, att_nbr, shift, m, inv, D and the out of the
 * gradients and of the row dot - is float32 [n, H], contiguous and head-minor: element node * H + h (the statistics of qgtc_heads.h).
 *
 * Contract. For every head h every output is, bit for bit, what the single-head entry gives on the contiguous slice of head h:
 * columns h * d .. of the node matrices as an [n, d] matrix, element [:, h] of the [n, H] vectors as an [n] vector. That holds plain,
 * under the edge-dropout mask and under the node masks. With heads = 1 an entry computes exactly its single-head twin.
 * `shift` of the forward is M[o, h], the largest att_nbr[k, h] over o's (kept, participating) neighbours: qgtc_tiledmax_f32 and its
 * _t / _drop / _nodes variants on att_nbr as an [n, H] matrix.
 *
 * Arguments: those of the single-head entry, then `int heads`, then the mask's arguments, then the stream. Refusals are the
 * single-head entry's in its order (invalid, then alignment, then size), with QGTC_EINVAL also for heads < 1 and for N % heads != 0;
 * the gradient entries, which run the heads (or groups of them) along a grid dimension, also refuse heads > 65535. The size checks of
 * the node matrices stay in elements (n * N); out_elems of the gradients and of the row dot is checked against n * heads.
 * Every element is written exactly once with a plain store; no atomics; one launch on the given stream; no host read. */
#ifndef QGTC_ATTN_HEADS_H
#define QGTC_ATTN_HEADS_H

#include "qgtc.h"

#ifdef __cplusplus
extern "C" {
#endif

int qgtc_tiledatt_heads_f32(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *X,
                            size_t x_elems, int N, const float *att_own, const float *att_nbr, float negative_slope, int backward,
                            const float *shift, float *m, float *inv, float *out, size_t out_elems, int heads, void *stream);
int qgtc_tiledatt_heads_f32_t(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                              int64_t n_tiles, int n, const float *X, size_t x_elems, int N, const float *att_own, const float *att_nbr,
                              float negative_slope, int backward, const float *shift, float *m, float *inv, float *out, size_t out_elems,
                              int heads, void *stream);
int qgtc_tiledatt_grad_heads_f32(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n,
                                 const float *A, const float *B, size_t ab_elems, int N, const float *att_own, const float *att_nbr,
                                 float negative_slope, int nbr_owns, const float *m, const float *inv, const float *D, float *out,
                                 size_t out_elems, int heads, void *stream);
int qgtc_tiledatt_grad_heads_f32_t(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                                   int64_t n_tiles, int n, const float *A, const float *B, size_t ab_elems, int N, const float *att_own,
                                   const float *att_nbr, float negative_slope, int nbr_owns, const float *m, const float *inv,
                                   const float *D, float *out, size_t out_elems, int heads, void *stream);
int qgtc_rowdot_heads_f32(const float *A, const float *B, size_t ab_elems, int n, int N, float *out, size_t out_elems, int heads,
                          void *stream);

int qgtc_tiledatt_heads_f32_drop(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n,
                                 const float *X, size_t x_elems, int N, const float *att_own, const float *att_nbr, float negative_slope,
                                 int backward, const float *shift, float *m, float *inv, float *out, size_t out_elems, int heads,
                                 uint32_t threshold, uint64_t seed, void *stream);
int qgtc_tiledatt_heads_f32_t_drop(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                                   int64_t n_tiles, int n, const float *X, size_t x_elems, int N, const float *att_own,
                                   const float *att_nbr, float negative_slope, int backward, const float *shift, float *m, float *inv,
                                   float *out, size_t out_elems, int heads, uint32_t threshold, uint64_t seed, void *stream);
int qgtc_tiledatt_grad_heads_f32_drop(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n,
                                      const float *A, const float *B, size_t ab_elems, int N, const float *att_own, const float *att_nbr,
                                      float negative_slope, int nbr_owns, const float *m, const float *inv, const float *D, float *out,
                                      size_t out_elems, int heads, uint32_t threshold, uint64_t seed, void *stream);
int qgtc_tiledatt_grad_heads_f32_t_drop(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                                        int64_t n_tiles, int n, const float *A, const float *B, size_t ab_elems, int N,
                                        const float *att_own, const float *att_nbr, float negative_slope, int nbr_owns, const float *m,
                                        const float *inv, const float *D, float *out, size_t out_elems, int heads, uint32_t threshold,
                                        uint64_t seed, void *stream);

int qgtc_tiledatt_heads_f32_nodes(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n,
                                  const float *X, size_t x_elems, int N, const float *att_own, const float *att_nbr, float negative_slope,
                                  int backward, const float *shift, float *m, float *inv, float *out, size_t out_elems, int heads,
                                  const uint32_t *row_mask, const uint32_t *nbr_mask, size_t mask_words, void *stream);
int qgtc_tiledatt_heads_f32_t_nodes(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                                    int64_t n_tiles, int n, const float *X, size_t x_elems, int N, const float *att_own,
                                    const float *att_nbr, float negative_slope, int backward, const float *shift, float *m, float *inv,
                                    float *out, size_t out_elems, int heads, const uint32_t *row_mask, const uint32_t *nbr_mask,
                                    size_t mask_words, void *stream);
int qgtc_tiledatt_grad_heads_f32_nodes(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n,
                                       const float *A, const float *B, size_t ab_elems, int N, const float *att_own, const float *att_nbr,
                                       float negative_slope, int nbr_owns, const float *m, const float *inv, const float *D, float *out,
                                       size_t out_elems, int heads, const uint32_t *row_mask, const uint32_t *nbr_mask,
                                       size_t mask_words, void *stream);
int qgtc_tiledatt_grad_heads_f32_t_nodes(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                                         int64_t n_tiles, int n, const float *A, const float *B, size_t ab_elems, int N,
                                         const float *att_own, const float *att_nbr, float negative_slope, int nbr_owns, const float *m,
                                         const float *inv, const float *D, float *out, size_t out_elems, int heads,
                                         const uint32_t *row_mask, const uint32_t *nbr_mask, size_t mask_words, void *stream);

#ifdef __cplusplus
}
#endif

#endif
