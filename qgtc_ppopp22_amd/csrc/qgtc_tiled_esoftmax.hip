// qgtc_tiled_esoftmax.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): the softmax of per-edge logits
// over each ROW's cells of the tile-compressed adjacency and its gradient, alpha[slot(i, j)] = EXP(l - m[i]) / den[i] (the row-view
// kernels of tiled_esoftmax_kernels.hip.h; include/qgtc.h, "Edge softmax"). A lane owns a row; nothing is
// shared between lanes, no atomics, every slot is written once. The entries for H heads in one launch (include/qgtc_heads.h; the kernels of
// tiled_heads_esoftmax_kernels.hip.h) are here too: the single-head entries are those with heads = 1.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "qgtc_heads.h"

#include "common.hip.h"
#include "tiled_float_kernels.hip.h"
#include "tiled_max_kernels.hip.h"   // tiled_static_for, for tiled_attn_kernels.hip.h (templates only: nothing is instantiated here)
#include "tiled_attn_kernels.hip.h"  // EXP and the unfused subtract and multiply
#include "tiled_esoftmax_kernels.hip.h"
#include "tiled_heads_esoftmax_kernels.hip.h"

int qgtc_tiled_edge_softmax_f32(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n,
                                const int64_t *val_ptr, const int16_t *val_row, const float *logits, float *alpha, size_t n_values,
                                float *m, float *inv, void *stream) {
    return tiled_esm_entry(TiledRowIndex{row_ptr, kquad}, tiles, n_tiles, n, val_ptr, val_row, logits, alpha, n_values, m, inv, 1, stream);
}

int qgtc_tiled_edge_softmax_heads_f32(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n,
                                      const int64_t *val_ptr, const int16_t *val_row, const float *logits, float *alpha,
                                      size_t n_values, float *m, float *inv, int heads, void *stream) {
    return tiled_esm_entry(TiledRowIndex{row_ptr, kquad}, tiles, n_tiles, n, val_ptr, val_row, logits, alpha, n_values, m, inv, heads, stream);
}

int qgtc_tiled_edge_softmax_grad_f32(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n,
                                     const int64_t *val_ptr, const int16_t *val_row, const float *alpha, const float *g, float *out,
                                     size_t n_values, void *stream) {
    return tiled_esm_grad_entry(TiledRowIndex{row_ptr, kquad}, tiles, n_tiles, n, val_ptr, val_row, alpha, g, out, n_values, 1, stream);
}

int qgtc_tiled_edge_softmax_grad_heads_f32(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n,
                                           const int64_t *val_ptr, const int16_t *val_row, const float *alpha, const float *g,
                                           float *out, size_t n_values, int heads, void *stream) {
    return tiled_esm_grad_entry(TiledRowIndex{row_ptr, kquad}, tiles, n_tiles, n, val_ptr, val_row, alpha, g, out, n_values, heads, stream);
}
