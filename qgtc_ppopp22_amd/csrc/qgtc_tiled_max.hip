// qgtc_tiled_max.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): the element-wise maximum / minimum
// over the neighbours of every row of the tile-compressed adjacency with the winner's id, and the select that is its gradient on this
// view (tiled_max_kernels.hip.h, which has their launcher).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "qgtc.h"

#include "common.hip.h"
#include "tiled_float_kernels.hip.h"
#include "tiled_max_kernels.hip.h"

int qgtc_tiledmax_f32(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *X,
                      size_t x_elems, int N, int op, float *out, size_t out_elems, int32_t *arg, size_t arg_elems,
                      void *stream) {
    const TiledRowIndex ix{row_ptr, kquad};
    const int rc = tiled_red_args_ok(ix.ok(), tiles, n_tiles, n, X, x_elems, N, out, out_elems, arg, arg_elems, false, op);
    if (rc != QGTC_OK) return rc;
    return tiled_extremum_run(ix, tiles, n_tiles, n, X, N, op, out, arg, stream);
}

int qgtc_tiledsel_f32(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *dY,
                      size_t dy_elems, int N, const int32_t *arg, size_t arg_elems, float *out, size_t out_elems, void *stream) {
    const TiledRowIndex ix{row_ptr, kquad};
    const int rc = tiled_red_args_ok(ix.ok(), tiles, n_tiles, n, dY, dy_elems, N, out, out_elems, arg, arg_elems, true, 0);
    if (rc != QGTC_OK) return rc;
    return tiled_red_f32_launch(ix, tiles, n_tiles, n, N, TiledSelect{dY, arg, out}, static_cast<hipStream_t>(stream));
}
