/* qgtc_addscore.h — the additive edge score of libqgtc_hip.so and its gradients (GATv2, Brody et al. 2022):
 * one score per stored cell and head of the tiled adjacency, att . leaky_relu(own[o] + nbr[k]), for H heads in ONE launch, and the two
 * folds of its backward. The terms - view, owner o, neighbours k ascending, slot, DOT's structure, fl = one IEEE single operation, never
 * fused - are those of "Attention tiled products" and "Edge values" in qgtc.h; the layout and the heads contract are those of
 * qgtc_heads.h. The ABI version of qgtc.h does not change: these are entries added beside it, declared in a header of their own.
 *
 * L(e) = e if e > 0 else fl(a * e), a = negative_slope in [0, 1]. N = H * d columns, head h = columns h d .. (h + 1) d - 1. att is
 * float32 [N]: head h's attention vector is att[h d .. (h + 1) d).
 *
 * Score. For one head of width d, rows x and y and the head's att:
 *   ADDSCORE(x, y; att): for j = 0 .. 63: t_j = +0; for c = j, j + 64, ... < d:
 *                            u = fl(x[c] + y[c]);  t_j = fl(t_j + fl(att[c] * L(u)))
 *                        then h = 32, 16, 8, 4, 2, 1: t_j = fl(t_j + t_(j xor h));  the result is t_0
 *   out[slot(i, j) * H + h] = ADDSCORE(A[i, head h], B[j, head h]; att[head h]) for every stored cell (i, j). Row view only: fl(x + y)
 *   commutes bit for bit, so on the other view the cell is the same one and the caller swaps A and B. Every (slot, head) is written
 *   exactly once with a plain store; no atomics.
 *
 * Gradients. g = dLoss/dscore is [n_values, H]. For an owner o of the view and a column c of head h, u_k = fl(own[o, c] + nbr[k, c]):
 *   FD[o, c] = fold over o's cells k ascending, from +0, of fl(acc + T),  T = g[slot, h] if u_k > 0 else fl(a * g[slot, h])
 *   FV[o, c] = fold over o's cells k ascending, from +0, of fl(acc + fl(g[slot, h] * L(u_k)))
 *   d_own[o, c] = fl(att[c] * FD[o, c])        P[o, c] = FV[o, c]
 * d_own is the gradient for the view's `own` operand; the gradient for `nbr` is the same entry on the OTHER view with the operands
 * swapped (u has the same bits there); the gradient for att is the column sum of P, left to the caller. The derivative at u = +-0 is
 * a. qgtc_tiled_addscore_grad_heads_f32 walks the rows of the adjacency, _t its columns. Either of d_own and P may be NULL, not both.
 *
 * Domain: finite inputs. A NaN or an infinity gives unspecified values in the cells and owners it reaches; nothing is read or written
 * out of bounds. For every head the result is, bit for bit, what heads = 1 gives on the head's contiguous slices.
 *
 * Refusals, before any device work, in the order invalid, alignment, size. The score entry: those of qgtc_tiled_sddmm_heads_f32; the
 * gradient entries: those of qgtc_tiledmm_f32_edge_heads (g in the place of values, d_own / P in the place of out). QGTC_EINVAL also
 * for a missing att, a slope outside [0, 1] or NaN, both outputs NULL, heads < 1 and N % heads != 0. QGTC_ESIZE in elements n * N; an
 * att_elems below N is QGTC_ESIZE too. n_tiles == 0 or n_values == 0 returns QGTC_OK; the gradient entries then fill d_own and P,
 * where given, with +0 on the stream. */
#ifndef QGTC_ADDSCORE_H
#define QGTC_ADDSCORE_H

#include "qgtc.h"

#ifdef __cplusplus
extern "C" {
#endif

int qgtc_tiled_addscore_heads_f32(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n,
                                  const float *A, const float *B, size_t ab_elems, int N, const float *att, size_t att_elems,
                                  float negative_slope, const int64_t *val_ptr, const int16_t *val_row, float *out, size_t n_values,
                                  int heads, void *stream);
int qgtc_tiled_addscore_grad_heads_f32(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n,
                                       const float *own, const float *nbr, size_t x_elems, int N, const float *att, size_t att_elems,
                                       float negative_slope, float *d_own, float *P, size_t out_elems, const int64_t *val_ptr,
                                       const int16_t *val_row, const float *g, size_t n_values, int heads, void *stream);
int qgtc_tiled_addscore_grad_heads_f32_t(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                                         int64_t n_tiles, int n, const float *own, const float *nbr, size_t x_elems, int N,
                                         const float *att, size_t att_elems, float negative_slope, float *d_own, float *P,
                                         size_t out_elems, const int64_t *val_ptr, const int16_t *val_row, const float *g,
                                         size_t n_values, int heads, void *stream);

#ifdef __cplusplus
}
#endif

#endif
