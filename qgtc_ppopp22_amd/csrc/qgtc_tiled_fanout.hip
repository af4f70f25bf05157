// qgtc_tiled_fanout.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): the selection launches of fixed-fanout
// neighbour sampling on both axes of the tile-compressed adjacency (tiled_fanout_kernels.hip.h; include/qgtc_fanout.h; DESIGN.md
// section 6.15l).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "qgtc_fanout.h"

#include "common.hip.h"
#include "tiled_fanout_kernels.hip.h"

int qgtc_tiled_fanout_thr(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, int k,
                          uint64_t seed, uint32_t *thr, size_t thr_elems, void *stream) {
    const TiledRowIndex ix{row_ptr, kquad};
    const int rc = tiled_fanout_thr_args_ok(ix.ok(), tiles, n_tiles, n, k, thr, thr_elems);
    if (rc != QGTC_OK) return rc;
    return tiled_fanout_thr_launch(FanoutRowWalk{row_ptr, kquad, tiles, static_cast<uint64_t>(n_tiles), n}, n, k, seed, thr, stream);
}

int qgtc_tiled_fanout_thr_t(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                            int64_t n_tiles, int n, int k, uint64_t seed, uint32_t *thr, size_t thr_elems, void *stream) {
    const TiledColIndex ix{col_ptr, col_tile, col_rb};
    const int rc = tiled_fanout_thr_args_ok(ix.ok(), tiles, n_tiles, n, k, thr, thr_elems);
    if (rc != QGTC_OK) return rc;
    return tiled_fanout_thr_launch(FanoutColWalk{col_ptr, col_tile, col_rb, tiles, static_cast<uint64_t>(n_tiles), n}, n, k, seed, thr,
                                   stream);
}
