// qgtc_tiled_float_t.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): the transposed product of the
// tile-compressed adjacency with a float32 right operand, out = A_tiled^T . X with an optional per-row scale
// (tiled_float_t_kernels.hip.h, which has its launcher).
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

int qgtc_tiledmm_f32_t(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles, int64_t n_tiles,
                       int n, const float *X, size_t x_elems, int N, const float *row_scale, float *out, size_t out_elems, void *stream) {
    const TiledColIndex ix{col_ptr, col_tile, col_rb};
    const int rc = tiled_f32_args_ok(ix.ok(), tiles, n_tiles, n, X, x_elems, N, row_scale, out, out_elems);
    if (rc != QGTC_OK) return rc;
    return tiled_mm_f32_run(ix, tiles, n_tiles, n, X, N, row_scale, out, stream);
}
