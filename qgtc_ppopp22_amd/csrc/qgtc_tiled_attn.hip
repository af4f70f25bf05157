// qgtc_tiled_attn.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): the softmax-weighted sum over the
// neighbours of every row of the tile-compressed adjacency and its gradients on this view (tiled_attn_kernels.hip.h, which has
// their launchers), and the row dot.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "qgtc.h"

#include "common.hip.h"
#include "tiled_float_kernels.hip.h"
#include "tiled_max_kernels.hip.h"   // tiled_static_for (templates only: nothing is instantiated here)
#include "tiled_attn_kernels.hip.h"

int qgtc_tiledatt_f32(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *X,
                      size_t x_elems, int N, const float *att_own, const float *att_nbr, float negative_slope, int backward,
                      const float *shift, float *m, float *inv, float *out, size_t out_elems, void *stream) {
    const TiledRowIndex ix{row_ptr, kquad};
    const int rc = tiled_att_f32_args_ok(ix.ok(), tiles, n_tiles, n, X, x_elems, N, att_own, att_nbr, negative_slope, backward, shift, m, inv, out,
                                         out_elems);
    if (rc != QGTC_OK) return rc;
    return tiled_att_f32_run(ix, tiles, n_tiles, n, X, N, att_own, att_nbr, negative_slope, backward, shift, m, inv, out, stream);
}

int qgtc_tiledatt_grad_f32(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *A,
                           const float *B, size_t ab_elems, int N, const float *att_own, const float *att_nbr, float negative_slope,
                           int nbr_owns, const float *m, const float *inv, const float *D, float *out, size_t out_elems, void *stream) {
    const TiledRowIndex ix{row_ptr, kquad};
    const int rc = tiled_att_grad_args_ok(ix.ok(), tiles, n_tiles, n, A, B, ab_elems, N, att_own, att_nbr, negative_slope, nbr_owns, m, inv, D, out,
                                          out_elems);
    if (rc != QGTC_OK) return rc;
    return tiled_att_grad_run(ix, tiles, n_tiles, n, A, B, N, att_own, att_nbr, negative_slope, nbr_owns, m, inv, D, out, stream);
}

int qgtc_rowdot_f32(const float *A, const float *B, size_t ab_elems, int n, int N, float *out, size_t out_elems, void *stream) {
    if (!A || !B || !out || n < 1 || n > TILED_MAX_N || N < 1) return QGTC_EINVAL;
    if (!aligned4(A) || !aligned4(B) || !aligned4(out)) return QGTC_EALIGN;
    if (ab_elems < static_cast<size_t>(n) * static_cast<size_t>(N) || out_elems < static_cast<size_t>(n)) return QGTC_ESIZE;
    hipLaunchKernelGGL(k_rowdot_f32, dim3((n + 3) / 4), dim3(256), 0, static_cast<hipStream_t>(stream), A, B, n, N, out);
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}
