/* qgtc_heads.h — the multi-head entries of libqgtc_hip.so's edge-value path: the per-edge dot (SDDMM), the weighted sum and the edge
 * softmax with its gradient, each for H heads in ONE launch. They generalise seven entries of qgtc.h ("Edge
 * values", "Edge softmax"), whose terms - slot, view, DOT, EXP, the order of every fold - are used here unchanged. The ABI version of
 * qgtc.h does not change: these are entries added beside it, declared in a header of their own until the two are folded together.
 *
 * Layout. A per-edge multi-head vector (scores, logits, alpha, their gradients, the weights of the sum) is float32 [n_values, H],
 * contiguous and head-minor, in SLOT order: the H values of one cell are adjacent, element slot * H + h. n_values stays the number of
 * stored cells. A node matrix is [n, N] with N = H * d and head h in the columns h * d .. (h + 1) * d - 1. The softmax statistics m
 * and inv are [n, H], element node * H + h.
 *
 * Contract. For every head h the result is, bit for bit, what the single-head entry gives on the contiguous slice of head h: columns
 * h * d .. of the node matrices as an [n, d] matrix, element [:, h] of the per-edge vectors as an [n_values] vector. With heads = 1 an
 * entry computes exactly its single-head twin.
 *
 *   qgtc_tiled_sddmm_heads_f32            out[slot(i, j) * H + h] = DOT over head h's d columns of A[i] and B[j]. Row view only.
 *   qgtc_tiledmm_f32_edge_heads / _t_..   out[i, c] = row_scale[i] . fold over i's neighbours j, ascending, of
 *                                         fl(acc + fl(values[slot * H + c / d] * X[j, c])).
 *   qgtc_tiled_edge_softmax_heads_f32 / _t, qgtc_tiled_edge_softmax_grad_heads_f32 / _t
 *                                         the forward and the gradient of "Edge softmax" per (owner, head); -inf, NaN and an owner
 *                                         without cells behave per head as they do there (m = +0 and inv = 0 in every head).
 * Every (slot, head) is written exactly once with a plain store; no atomics.
 *
 * Arguments: those of the single-head entry, then `int heads` before the stream. Refusals are the single-head entry's in its order
 * (invalid, then alignment, then size), with QGTC_EINVAL also for heads < 1 and, where there is an N, for N % heads != 0; the softmax
 * entries, which have no N, refuse heads > 65535 (the heads ride a grid dimension). The size checks stay in elements of the node
 * matrices (n * N); n_values above 2^31 - 1 is QGTC_EINVAL as before. */
#ifndef QGTC_HEADS_H
#define QGTC_HEADS_H

#include "qgtc.h"

#ifdef __cplusplus
extern "C" {
#endif

int qgtc_tiled_sddmm_heads_f32(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n,
                               const float *A, const float *B, size_t ab_elems, int N, const int64_t *val_ptr, const int16_t *val_row,
                               float *out, size_t n_values, int heads, void *stream);
int qgtc_tiledmm_f32_edge_heads(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n,
                                const float *X, size_t x_elems, int N, const float *row_scale, float *out, size_t out_elems,
                                const int64_t *val_ptr, const int16_t *val_row, const float *values, size_t n_values, int heads,
                                void *stream);
int qgtc_tiledmm_f32_t_edge_heads(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                                  int64_t n_tiles, int n, const float *X, size_t x_elems, int N, const float *row_scale, float *out,
                                  size_t out_elems, const int64_t *val_ptr, const int16_t *val_row, const float *values,
                                  size_t n_values, int heads, void *stream);
int qgtc_tiled_edge_softmax_heads_f32(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n,
                                      const int64_t *val_ptr, const int16_t *val_row, const float *logits, float *alpha,
                                      size_t n_values, float *m, float *inv, int heads, void *stream);
int qgtc_tiled_edge_softmax_heads_f32_t(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                                        int64_t n_tiles, int n, const int64_t *val_ptr, const int16_t *val_row, const float *logits,
                                        float *alpha, size_t n_values, float *m, float *inv, int heads, void *stream);
int qgtc_tiled_edge_softmax_grad_heads_f32(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n,
                                           const int64_t *val_ptr, const int16_t *val_row, const float *alpha, const float *g,
                                           float *out, size_t n_values, int heads, void *stream);
int qgtc_tiled_edge_softmax_grad_heads_f32_t(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb,
                                             const uint32_t *tiles, int64_t n_tiles, int n, const int64_t *val_ptr,
                                             const int16_t *val_row, const float *alpha, const float *g, float *out, size_t n_values,
                                             int heads, void *stream);

#ifdef __cplusplus
}
#endif

#endif
