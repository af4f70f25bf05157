// qgtc_tiled_max_fanout_nodes.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): the element-wise maximum /
// minimum over the neighbours a fixed-fanout sample of an induced subgraph keeps, on both views of the tile-compressed adjacency (the
// instantiations of tiled_max_kernels.hip.h and tiled_max_t_kernels.hip.h with the fanout mask, own and nbr form, and then the node
// masks; include/qgtc_blocks.h). The select needs no mask: arg names kept neighbours only.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "qgtc_blocks.h"

#include "common.hip.h"
#include "tiled_fanout.hip.h"
#include "bitmm_popcount.hip.h"   // requant, for tiled_t_kernels.hip.h (templates only: nothing is instantiated here)
#include "tiled_t_kernels.hip.h"  // the in-register bit transpose
#include "tiled_float_kernels.hip.h"
#include "tiled_max_kernels.hip.h"
#include "tiled_max_t_kernels.hip.h"

int qgtc_tiledmax_f32_fanout_nodes(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n,
                                   const float *X, size_t x_elems, int N, int op, float *out, size_t out_elems, int32_t *arg,
                                   size_t arg_elems, const uint32_t *thr, int thr_of_nbr, uint64_t seed, const uint32_t *row_mask,
                                   const uint32_t *nbr_mask, size_t mask_words, void *stream) {
    const TiledRowIndex ix{row_ptr, kquad};
    int rc = tiled_fanout_args_ok(tiled_red_args_ok(ix.ok(), tiles, n_tiles, n, X, x_elems, N, out, out_elems, arg, arg_elems, false, op), thr,
                                  thr_of_nbr);
    if (rc == QGTC_OK) rc = tiled_nodes_args_ok(row_mask, nbr_mask, mask_words, n);
    if (rc != QGTC_OK) return rc;
    return tiled_fanout_run<false>(thr, thr_of_nbr, seed, n, [&](auto mask) {
        return tiled_extremum_run(ix, tiles, n_tiles, n, X, N, op, out, arg, stream, mask, TiledNodes{row_mask, nbr_mask});
    });
}

int qgtc_tiledmax_f32_t_fanout_nodes(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                                     int64_t n_tiles, int n, const float *X, size_t x_elems, int N, int op, float *out, size_t out_elems,
                                     int32_t *arg, size_t arg_elems, const uint32_t *thr, int thr_of_nbr, uint64_t seed,
                                     const uint32_t *row_mask, const uint32_t *nbr_mask, size_t mask_words, void *stream) {
    const TiledColIndex ix{col_ptr, col_tile, col_rb};
    int rc = tiled_fanout_args_ok(tiled_red_args_ok(ix.ok(), tiles, n_tiles, n, X, x_elems, N, out, out_elems, arg, arg_elems, false, op), thr,
                                  thr_of_nbr);
    if (rc == QGTC_OK) rc = tiled_nodes_args_ok(row_mask, nbr_mask, mask_words, n);
    if (rc != QGTC_OK) return rc;
    return tiled_fanout_run<true>(thr, thr_of_nbr, seed, n, [&](auto mask) {
        return tiled_extremum_run(ix, tiles, n_tiles, n, X, N, op, out, arg, stream, mask, TiledNodes{row_mask, nbr_mask});
    });
}
