// qgtc_tiled_float_edge_heads.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): the float product of the
// tile-compressed adjacency with a value per stored cell and head, out[i, c] = row_scale[i] . sum_j values[slot(i, j) * H + c / d] .
// X[j, c] (the row-view kernel of tiled_heads_mm_kernels.hip.h; include/qgtc_heads.h).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "qgtc_heads.h"

#include "common.hip.h"
#include "tiled_float_kernels.hip.h"
#include "tiled_heads_mm_kernels.hip.h"

int qgtc_tiledmm_f32_edge_heads(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n,
                                const float *X, size_t x_elems, int N, const float *row_scale, float *out, size_t out_elems,
                                const int64_t *val_ptr, const int16_t *val_row, const float *values, size_t n_values, int heads,
                                void *stream) {
    if (heads == 1)   // the single-head kernel (qgtc_tiled_float_edge.hip), with the same refusals
        return qgtc_tiledmm_f32_edge(row_ptr, kquad, tiles, n_tiles, n, X, x_elems, N, row_scale, out, out_elems, val_ptr, val_row, values,
                                     n_values, stream);
    return tiled_mm_f32_heads_entry(TiledRowIndex{row_ptr, kquad}, tiles, n_tiles, n, X, x_elems, N, row_scale, out, out_elems, val_ptr,
                                    val_row, values, n_values, heads, stream);
}
