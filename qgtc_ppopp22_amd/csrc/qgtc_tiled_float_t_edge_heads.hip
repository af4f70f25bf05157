// qgtc_tiled_float_t_edge_heads.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): the transposed float
// product of the tile-compressed adjacency with a value per stored cell and head, out[j, c] = row_scale[j] . sum_i values[slot(i, j) * H
// + c / d] . X[i, c] (the column-view kernel of tiled_heads_mm_kernels.hip.h; include/qgtc_heads.h). The
// values are the row view's array: a cell's slot does not depend on the view.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "qgtc_heads.h"

#include "common.hip.h"
#include "bitmm_popcount.hip.h"   // requant, for tiled_t_kernels.hip.h (templates only: nothing is instantiated here)
#include "tiled_t_kernels.hip.h"  // the in-register bit transpose
#include "tiled_float_kernels.hip.h"
#define QGTC_TILED_HEADS_T 1      // the column view's kernel of the shared header
#include "tiled_heads_mm_kernels.hip.h"

int qgtc_tiledmm_f32_t_edge_heads(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                                  int64_t n_tiles, int n, const float *X, size_t x_elems, int N, const float *row_scale, float *out,
                                  size_t out_elems, const int64_t *val_ptr, const int16_t *val_row, const float *values,
                                  size_t n_values, int heads, void *stream) {
    if (heads == 1)   // the single-head kernel (qgtc_tiled_float_t_edge.hip), with the same refusals
        return qgtc_tiledmm_f32_t_edge(col_ptr, col_tile, col_rb, tiles, n_tiles, n, X, x_elems, N, row_scale, out, out_elems, val_ptr,
                                       val_row, values, n_values, stream);
    return tiled_mm_f32_heads_entry(TiledColIndex{col_ptr, col_tile, col_rb}, tiles, n_tiles, n, X, x_elems, N, row_scale, out, out_elems,
                                    val_ptr, val_row, values, n_values, heads, stream);
}
