// qgtc_tiled_attn_heads.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): the softmax-weighted sum over the neighbours of every row of the
// tile-compressed adjacency and its gradients for H heads in one launch, on the row view (the instantiations of
// tiled_attn_heads_kernels.hip.h; include/qgtc_attn_heads.h; include/qgtc.h, "Attention tiled products").
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

int qgtc_tiledatt_heads_f32(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *X, size_t x_elems, int N, const float *att_own, const float *att_nbr,
        float negative_slope, int backward, const float *shift, float *m, float *inv, float *out, size_t out_elems, int heads,
        void *stream) {
    const TiledRowIndex ix{row_ptr, kquad};
    int rc = tiled_atth_f32_args_ok(ix.ok(), tiles, n_tiles, n, X, x_elems, N, att_own, att_nbr, negative_slope, backward, shift, m, inv, out,
                                    out_elems, heads);
    if (rc != QGTC_OK) return rc;
    return tiled_atth_f32_run(ix, tiles, n_tiles, n, X, N, att_own, att_nbr, negative_slope, backward, shift, m, inv, out, heads, stream);
}

int qgtc_tiledatt_grad_heads_f32(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *A, const float *B, size_t ab_elems, int N, const float *att_own,
        const float *att_nbr, float negative_slope, int nbr_owns, const float *m, const float *inv, const float *D, float *out,
        size_t out_elems, int heads, void *stream) {
    const TiledRowIndex ix{row_ptr, kquad};
    int rc = tiled_atth_grad_args_ok(ix.ok(), tiles, n_tiles, n, A, B, ab_elems, N, att_own, att_nbr, negative_slope, nbr_owns, m, inv, D, out,
                                     out_elems, heads);
    if (rc != QGTC_OK) return rc;
    return tiled_atth_grad_run(ix, tiles, n_tiles, n, A, B, N, att_own, att_nbr, negative_slope, nbr_owns, m, inv, D, out, heads, stream);
}

int qgtc_rowdot_heads_f32(const float *A, const float *B, size_t ab_elems, int n, int N, float *out, size_t out_elems, int heads,
                          void *stream) {
    if (!A || !B || !out || n < 1 || n > TILED_MAX_N || N < 1 || heads < 1 || N % heads != 0) return QGTC_EINVAL;
    if (!aligned4(A) || !aligned4(B) || !aligned4(out)) return QGTC_EALIGN;
    if (ab_elems < static_cast<size_t>(n) * static_cast<size_t>(N) || out_elems < static_cast<size_t>(n) * static_cast<size_t>(heads))
        return QGTC_ESIZE;
    const TiledAttHShape sh = tiled_atth_shape(heads, N / heads);
    const TiledAttH at{TiledAtt{nullptr, nullptr, nullptr, nullptr, nullptr, 0.0f}, heads, N / heads, sh.lg};
    const int per_row = sh.wide ? heads : sh.slots;   // waves a row takes
    const uint64_t blocks = (static_cast<uint64_t>(n) * static_cast<uint64_t>(per_row) + 3) / 4;
    if (blocks > 0x7fffffffull) return QGTC_EINVAL;
    const dim3 grid(static_cast<unsigned>(blocks)), block(256);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (sh.wide) hipLaunchKernelGGL(k_rowdot_heads_f32<true>, grid, block, 0, st, A, B, n, N, at, per_row, out);
    else hipLaunchKernelGGL(k_rowdot_heads_f32<false>, grid, block, 0, st, A, B, n, N, at, per_row, out);
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}
