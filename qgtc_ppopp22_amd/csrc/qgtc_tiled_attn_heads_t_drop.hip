// qgtc_tiled_attn_heads_t_drop.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): the softmax-weighted sum over the neighbours the edge-dropout mask keeps, of every row of the
// tile-compressed adjacency and its gradients for H heads in one launch, on the column view (A^T) (the instantiations of
// tiled_attn_heads_t_kernels.hip.h with the mask; include/qgtc_attn_heads.h; include/qgtc.h, "Edge dropout").
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "qgtc_attn_heads.h"

#include "common.hip.h"
#include "bitmm_popcount.hip.h"   // requant, for tiled_t_kernels.hip.h (templates only: nothing is instantiated here)
#include "tiled_t_kernels.hip.h"  // the in-register bit transpose
#include "tiled_float_kernels.hip.h"
#include "tiled_max_kernels.hip.h"   // tiled_static_for
#include "tiled_attn_kernels.hip.h"  // the arithmetic of the single-head kernels (templates only)
#include "tiled_attn_t_kernels.hip.h"   // the transposer role
#include "tiled_attn_heads_kernels.hip.h"
#include "tiled_attn_heads_t_kernels.hip.h"

int qgtc_tiledatt_heads_f32_t_drop(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles, int64_t n_tiles, int n, const float *X, size_t x_elems, int N, const float *att_own, const float *att_nbr,
        float negative_slope, int backward, const float *shift, float *m, float *inv, float *out, size_t out_elems, int heads, uint32_t threshold, uint64_t seed,
        void *stream) {
    const TiledColIndex ix{col_ptr, col_tile, col_rb};
    int rc = tiled_atth_f32_args_ok(ix.ok(), tiles, n_tiles, n, X, x_elems, N, att_own, att_nbr, negative_slope, backward, shift, m, inv, out,
                                    out_elems, heads);
    if (rc != QGTC_OK) return rc;
    return tiled_atth_f32_run(ix, tiles, n_tiles, n, X, N, att_own, att_nbr, negative_slope, backward, shift, m, inv, out, heads, stream, TiledDropView<true>{tiled_drop_make(threshold, seed)});
}

int qgtc_tiledatt_grad_heads_f32_t_drop(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles, int64_t n_tiles, int n, const float *A, const float *B, size_t ab_elems, int N, const float *att_own,
        const float *att_nbr, float negative_slope, int nbr_owns, const float *m, const float *inv, const float *D, float *out,
        size_t out_elems, int heads, uint32_t threshold, uint64_t seed, void *stream) {
    const TiledColIndex ix{col_ptr, col_tile, col_rb};
    int rc = tiled_atth_grad_args_ok(ix.ok(), tiles, n_tiles, n, A, B, ab_elems, N, att_own, att_nbr, negative_slope, nbr_owns, m, inv, D, out,
                                     out_elems, heads);
    if (rc != QGTC_OK) return rc;
    return tiled_atth_grad_run(ix, tiles, n_tiles, n, A, B, N, att_own, att_nbr, negative_slope, nbr_owns, m, inv, D, out, heads, stream, TiledDropView<true>{tiled_drop_make(threshold, seed)});
}
