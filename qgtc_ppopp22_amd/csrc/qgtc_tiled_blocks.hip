// qgtc_tiled_blocks.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): the selection launches of fixed-fanout
// sampling on an induced subgraph, on both axes, and the frontier of such a sample as a node bitmap (tiled_blocks_kernels.hip.h;
// include/qgtc_blocks.h).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "qgtc_blocks.h"

#include "common.hip.h"
#include "tiled_blocks_kernels.hip.h"

int qgtc_tiled_fanout_thr_nodes(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, int k,
                                uint64_t seed, uint32_t *thr, size_t thr_elems, int32_t *kept, size_t kept_elems,
                                const uint32_t *row_mask, const uint32_t *nbr_mask, size_t mask_words, void *stream) {
    const TiledRowIndex ix{row_ptr, kquad};
    const int rc = tiled_fanout_thr_nodes_args_ok(ix.ok(), tiles, n_tiles, n, k, thr, thr_elems, kept, kept_elems, row_mask, nbr_mask,
                                                  mask_words);
    if (rc != QGTC_OK) return rc;
    const FanoutRowWalkNodes walk{FanoutRowWalk{row_ptr, kquad, tiles, static_cast<uint64_t>(n_tiles), n}, nbr_mask};
    return tiled_fanout_thr_nodes_launch(walk, n, k, seed, row_mask, thr, kept, stream);
}

int qgtc_tiled_fanout_thr_t_nodes(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                                  int64_t n_tiles, int n, int k, uint64_t seed, uint32_t *thr, size_t thr_elems, int32_t *kept,
                                  size_t kept_elems, const uint32_t *row_mask, const uint32_t *nbr_mask, size_t mask_words, void *stream) {
    const TiledColIndex ix{col_ptr, col_tile, col_rb};
    const int rc = tiled_fanout_thr_nodes_args_ok(ix.ok(), tiles, n_tiles, n, k, thr, thr_elems, kept, kept_elems, row_mask, nbr_mask,
                                                  mask_words);
    if (rc != QGTC_OK) return rc;
    const FanoutColWalkNodes walk{FanoutColWalk{col_ptr, col_tile, col_rb, tiles, static_cast<uint64_t>(n_tiles), n}, nbr_mask};
    return tiled_fanout_thr_nodes_launch(walk, n, k, seed, row_mask, thr, kept, stream);
}

int qgtc_tiled_fanout_frontier(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                               int64_t n_tiles, int n, const uint32_t *thr, uint64_t seed, const uint32_t *row_mask,
                               const uint32_t *nbr_mask, const uint32_t *include, size_t mask_words, uint32_t *out, size_t out_words,
                               void *stream) {
    const TiledColIndex ix{col_ptr, col_tile, col_rb};
    const int rc = tiled_fanout_frontier_args_ok(ix.ok(), tiles, n_tiles, n, thr, row_mask, nbr_mask, include, mask_words, out, out_words);
    if (rc != QGTC_OK) return rc;
    hipLaunchKernelGGL(k_tiled_fanout_frontier, dim3(step128(n)), dim3(256), 0, static_cast<hipStream_t>(stream), col_ptr, col_tile, col_rb,
                       tiles, static_cast<uint64_t>(n_tiles), n, tiled_drop_make(0u, seed), thr, row_mask, nbr_mask, include, out);
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

int qgtc_tiled_fanout_frontier_t(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n,
                                 const uint32_t *thr, uint64_t seed, const uint32_t *row_mask, const uint32_t *nbr_mask,
                                 const uint32_t *include, size_t mask_words, uint32_t *out, size_t out_words, void *stream) {
    const TiledRowIndex ix{row_ptr, kquad};
    const int rc = tiled_fanout_frontier_args_ok(ix.ok(), tiles, n_tiles, n, thr, row_mask, nbr_mask, include, mask_words, out, out_words);
    if (rc != QGTC_OK) return rc;
    hipLaunchKernelGGL(k_tiled_fanout_frontier_t, dim3(step128(n) * 4), dim3(256), 0, static_cast<hipStream_t>(stream), row_ptr, kquad, tiles,
                       static_cast<uint64_t>(n_tiles), n, tiled_drop_make(0u, seed), thr, row_mask, nbr_mask, include, out);
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}
