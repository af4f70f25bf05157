// qgtc_tiled_float_src.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): the float product of the
// tile-compressed adjacency with a scale on the SOURCE row, out = diag(row_scale) . A_tiled . diag(src_scale) . X (the instantiations
// of tiled_float_kernels.hip.h with a source scale).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "qgtc.h"

#include "common.hip.h"
#include "tiled_float_kernels.hip.h"

int qgtc_tiledmm_f32_src(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *X,
                         size_t x_elems, int N, const float *row_scale, const float *src_scale, float *out, size_t out_elems,
                         void *stream) {
    if (!src_scale) return qgtc_tiledmm_f32(row_ptr, kquad, tiles, n_tiles, n, X, x_elems, N, row_scale, out, out_elems, stream);
    const TiledRowIndex ix{row_ptr, kquad};
    const int rc = tiled_f32_args_ok(ix.ok(), tiles, n_tiles, n, X, x_elems, N, row_scale, out, out_elems, src_scale);
    if (rc != QGTC_OK) return rc;
    return tiled_mm_f32_run(ix, tiles, n_tiles, n, X, N, row_scale, out, stream, src_scale);
}
