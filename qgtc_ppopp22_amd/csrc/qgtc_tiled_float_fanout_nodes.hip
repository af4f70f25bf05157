// qgtc_tiled_float_fanout_nodes.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): the float product of the
// tile-compressed adjacency over a fixed-fanout sample of an induced subgraph (the instantiations of tiled_float_kernels.hip.h whose pack
// ends in the fanout mask, own and nbr form, and then the node masks; include/qgtc_blocks.h). The kernel body is
// unchanged: it asks the pack's FIRST mask element per neighbour (the sample) and finds the node masks wherever they stand.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "qgtc_blocks.h"

#include "common.hip.h"
#include "tiled_fanout.hip.h"
#include "tiled_float_kernels.hip.h"

int qgtc_tiledmm_f32_fanout_nodes(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n,
                                  const float *X, size_t x_elems, int N, const float *row_scale, const float *src_scale, float *out,
                                  size_t out_elems, const uint32_t *thr, int thr_of_nbr, uint64_t seed, const uint32_t *row_mask,
                                  const uint32_t *nbr_mask, size_t mask_words, void *stream) {
    const TiledRowIndex ix{row_ptr, kquad};
    int rc = tiled_fanout_args_ok(tiled_f32_args_ok(ix.ok(), tiles, n_tiles, n, X, x_elems, N, row_scale, out, out_elems, src_scale), thr,
                                  thr_of_nbr);
    if (rc == QGTC_OK) rc = tiled_nodes_args_ok(row_mask, nbr_mask, mask_words, n);
    if (rc != QGTC_OK) return rc;
    const TiledNodes nodes{row_mask, nbr_mask};
    return tiled_fanout_run<false>(thr, thr_of_nbr, seed, n, [&](auto mask) {
        return src_scale ? tiled_mm_f32_run(ix, tiles, n_tiles, n, X, N, row_scale, out, stream, src_scale, mask, nodes)
                         : tiled_mm_f32_run(ix, tiles, n_tiles, n, X, N, row_scale, out, stream, mask, nodes);
    });
}
