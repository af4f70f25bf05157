// qgtc_tiled_float_t_nodes.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): the transposed float
// product of the tile-compressed adjacency under node masks, out = diag(row_scale) . (A_tiled^T restricted to row_mask x nbr_mask) .
// diag(src_scale) . X (the instantiations of tiled_float_t_kernels.hip.h whose pack ends in the masks; include/qgtc.h, "Node masks";
// DESIGN.md section 6.15e). The masks are relative to the view: row_mask names output rows (A's columns).
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

int qgtc_tiledmm_f32_t_nodes(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                             int64_t n_tiles, int n, const float *X, size_t x_elems, int N, const float *row_scale,
                             const float *src_scale, float *out, size_t out_elems, const uint32_t *row_mask, const uint32_t *nbr_mask,
                             size_t mask_words, void *stream) {
    const TiledColIndex ix{col_ptr, col_tile, col_rb};
    int rc = tiled_f32_args_ok(ix.ok(), tiles, n_tiles, n, X, x_elems, N, row_scale, out, out_elems, src_scale);
    if (rc == QGTC_OK) rc = tiled_nodes_args_ok(row_mask, nbr_mask, mask_words, n);
    if (rc != QGTC_OK) return rc;
    return tiled_mm_f32_masked(ix, tiles, n_tiles, n, X, N, row_scale, src_scale, out, stream, TiledNodes{row_mask, nbr_mask});
}
