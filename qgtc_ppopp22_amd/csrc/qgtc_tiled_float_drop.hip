// qgtc_tiled_float_drop.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): the float product of the
// tile-compressed adjacency under the edge-dropout mask, out = diag(row_scale) . (A_tiled masked) . diag(src_scale) . X (the
// instantiations of tiled_float_kernels.hip.h whose pack ends in the mask; include/qgtc.h, "Edge dropout"),
// and the host-side keep test.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "qgtc.h"

#include "common.hip.h"
#include "tiled_float_kernels.hip.h"

int qgtc_tiledmm_f32_drop(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *X,
                          size_t x_elems, int N, const float *row_scale, const float *src_scale, float *out, size_t out_elems,
                          uint32_t threshold, uint64_t seed, void *stream) {
    const TiledRowIndex ix{row_ptr, kquad};
    const int rc = tiled_f32_args_ok(ix.ok(), tiles, n_tiles, n, X, x_elems, N, row_scale, out, out_elems, src_scale);
    if (rc != QGTC_OK) return rc;
    return tiled_mm_f32_masked(ix, tiles, n_tiles, n, X, N, row_scale, src_scale, out, stream,
                               TiledDropView<false>{tiled_drop_make(threshold, seed)});
}

// the keep test on the host: the functions the kernels run (tiled_drop.hip.h)
int qgtc_edge_kept(uint32_t i, uint32_t j, uint64_t seed, uint32_t threshold) {
    const TiledDrop d = tiled_drop_make(threshold, seed);
    return tiled_drop_test(d, tiled_drop_row_half(d, i), tiled_drop_col_half(d, j)) ? 1 : 0;
}
