// qgtc_tiled_float_t_edge.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): the transposed float product
// of the tile-compressed adjacency with a value per stored cell, out[j] = row_scale[j] . sum_i values[slot(i, j)] . X[i] (the
// instantiations of tiled_float_t_kernels.hip.h whose pack ends in the edge values; include/qgtc.h, "Edge values"; DESIGN.md section
// 6.15g). The values are the row view's array: a cell's slot does not depend on the view.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "qgtc.h"

#include "common.hip.h"
#include "bitmm_popcount.hip.h"   // requant, for tiled_t_kernels.hip.h (templates only: nothing is instantiated here)
#include "tiled_t_kernels.hip.h"  // the in-register bit transpose
#include "tiled_float_kernels.hip.h"
#include "tiled_float_t_kernels.hip.h"

int qgtc_tiledmm_f32_t_edge(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                            int64_t n_tiles, int n, const float *X, size_t x_elems, int N, const float *row_scale, float *out,
                            size_t out_elems, const int64_t *val_ptr, const int16_t *val_row, const float *values, size_t n_values,
                            void *stream) {
    const TiledColIndex ix{col_ptr, col_tile, col_rb};
    const int rc = tiled_edge_rc(tiled_f32_args_ok(ix.ok(), tiles, n_tiles, n, X, x_elems, N, row_scale, out, out_elems, values),
                                 n_tiles > 0 && !values ? QGTC_EINVAL : tiled_edge_index_ok(val_ptr, val_row, n_tiles, n_values));
    if (rc != QGTC_OK) return rc;
    return tiled_mm_f32_run(ix, tiles, n_tiles, n, X, N, row_scale, out, stream, TiledEdge{val_ptr, val_row, values, static_cast<int>(n_values)});
}
