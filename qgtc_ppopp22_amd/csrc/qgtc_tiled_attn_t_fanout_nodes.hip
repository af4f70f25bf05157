// qgtc_tiled_attn_t_fanout_nodes.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): the softmax-weighted sum
// over the neighbours a fixed-fanout sample of an induced subgraph keeps, of every column of the tile-compressed adjacency, and its
// gradients on this view (the instantiations of tiled_attn_t_kernels.hip.h with the fanout mask, own and nbr form, and then the node
// masks; include/qgtc_blocks.h).
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
#include "tiled_max_kernels.hip.h"   // tiled_static_for
#include "tiled_attn_kernels.hip.h"
#include "tiled_attn_t_kernels.hip.h"

int qgtc_tiledatt_f32_t_fanout_nodes(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                                     int64_t n_tiles, int n, const float *X, size_t x_elems, int N, const float *att_own,
                                     const float *att_nbr, float negative_slope, int backward, const float *shift, float *m, float *inv,
                                     float *out, size_t out_elems, const uint32_t *thr, int thr_of_nbr, uint64_t seed,
                                     const uint32_t *row_mask, const uint32_t *nbr_mask, size_t mask_words, void *stream) {
    const TiledColIndex ix{col_ptr, col_tile, col_rb};
    int rc = tiled_fanout_args_ok(tiled_att_f32_args_ok(ix.ok(), tiles, n_tiles, n, X, x_elems, N, att_own, att_nbr, negative_slope, backward,
                                                        shift, m, inv, out, out_elems),
                                  thr, thr_of_nbr);
    if (rc == QGTC_OK) rc = tiled_nodes_args_ok(row_mask, nbr_mask, mask_words, n);
    if (rc != QGTC_OK) return rc;
    return tiled_fanout_run<true>(thr, thr_of_nbr, seed, n, [&](auto mask) {
        return tiled_att_f32_run(ix, tiles, n_tiles, n, X, N, att_own, att_nbr, negative_slope, backward, shift, m, inv, out, stream, mask,
                                 TiledNodes{row_mask, nbr_mask});
    });
}

int qgtc_tiledatt_grad_f32_t_fanout_nodes(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                                          int64_t n_tiles, int n, const float *A, const float *B, size_t ab_elems, int N,
                                          const float *att_own, const float *att_nbr, float negative_slope, int nbr_owns, const float *m,
                                          const float *inv, const float *D, float *out, size_t out_elems, const uint32_t *thr,
                                          int thr_of_nbr, uint64_t seed, const uint32_t *row_mask, const uint32_t *nbr_mask,
                                          size_t mask_words, void *stream) {
    const TiledColIndex ix{col_ptr, col_tile, col_rb};
    int rc = tiled_fanout_args_ok(tiled_att_grad_args_ok(ix.ok(), tiles, n_tiles, n, A, B, ab_elems, N, att_own, att_nbr, negative_slope,
                                                         nbr_owns, m, inv, D, out, out_elems),
                                  thr, thr_of_nbr);
    if (rc == QGTC_OK) rc = tiled_nodes_args_ok(row_mask, nbr_mask, mask_words, n);
    if (rc != QGTC_OK) return rc;
    return tiled_fanout_run<true>(thr, thr_of_nbr, seed, n, [&](auto mask) {
        return tiled_att_grad_run(ix, tiles, n_tiles, n, A, B, N, att_own, att_nbr, negative_slope, nbr_owns, m, inv, D, out, stream, mask,
                                  TiledNodes{row_mask, nbr_mask});
    });
}
