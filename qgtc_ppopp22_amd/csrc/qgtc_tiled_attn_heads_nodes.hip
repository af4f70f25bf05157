// qgtc_tiled_attn_heads_nodes.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): the softmax-weighted sum over the neighbours in nbr_mask, of the rows in row_mask of the
// tile-compressed adjacency and its gradients for H heads in one launch, on the row view (the instantiations of
// tiled_attn_heads_kernels.hip.h with the mask; include/qgtc_attn_heads.h; include/qgtc.h, "Node masks").
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "qgtc_attn_heads.h"

#include "common.hip.h"
#include "tiled_float_kernels.hip.h"
#include "tiled_max_kernels.hip.h"   // tiled_static_for (templates only: nothing is instantiated here)
#include "tiled_attn_kernels.hip.h"  // the arithmetic of the single-head kernels (templates only)
#include "tiled_attn_heads_kernels.hip.h"

int qgtc_tiledatt_heads_f32_nodes(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *X, size_t x_elems, int N, const float *att_own, const float *att_nbr,
        float negative_slope, int backward, const float *shift, float *m, float *inv, float *out, size_t out_elems, int heads, const uint32_t *row_mask, const uint32_t *nbr_mask, size_t mask_words,
        void *stream) {
    const TiledRowIndex ix{row_ptr, kquad};
    int rc = tiled_atth_f32_args_ok(ix.ok(), tiles, n_tiles, n, X, x_elems, N, att_own, att_nbr, negative_slope, backward, shift, m, inv, out,
                                    out_elems, heads);
    if (rc == QGTC_OK) rc = tiled_nodes_args_ok(row_mask, nbr_mask, mask_words, n);
    if (rc != QGTC_OK) return rc;
    return tiled_atth_f32_run(ix, tiles, n_tiles, n, X, N, att_own, att_nbr, negative_slope, backward, shift, m, inv, out, heads, stream, TiledNodes{row_mask, nbr_mask});
}

int qgtc_tiledatt_grad_heads_f32_nodes(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *A, const float *B, size_t ab_elems, int N, const float *att_own,
        const float *att_nbr, float negative_slope, int nbr_owns, const float *m, const float *inv, const float *D, float *out,
        size_t out_elems, int heads, const uint32_t *row_mask, const uint32_t *nbr_mask, size_t mask_words, void *stream) {
    const TiledRowIndex ix{row_ptr, kquad};
    int rc = tiled_atth_grad_args_ok(ix.ok(), tiles, n_tiles, n, A, B, ab_elems, N, att_own, att_nbr, negative_slope, nbr_owns, m, inv, D, out,
                                     out_elems, heads);
    if (rc == QGTC_OK) rc = tiled_nodes_args_ok(row_mask, nbr_mask, mask_words, n);
    if (rc != QGTC_OK) return rc;
    return tiled_atth_grad_run(ix, tiles, n_tiles, n, A, B, N, att_own, att_nbr, negative_slope, nbr_owns, m, inv, D, out, heads, stream, TiledNodes{row_mask, nbr_mask});
}
