// qgtc_tiled_attn.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): the softmax-weighted sum over the
// neighbours of every row of the tile-compressed adjacency and its gradients on this view (tiled_attn_kernels.hip.h), the row dot, and
// their launchers.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "qgtc.h"

#include "common.hip.h"
#include "tiled_float_kernels.hip.h"
#include "tiled_max_kernels.hip.h"   // tiled_static_for (templates only: nothing is instantiated here)
#include "tiled_attn_kernels.hip.h"

namespace {

// lanes per output row and columns per lane by N: the float product's choice (qgtc_tiled_float.hip; tests/tiled_attn_model.py,
// ATT_FORWARD_VARIANTS, states the same)
template <bool BWD>
int tiled_att_f32(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *X, int N,
                  const TiledAtt &att, float *m, float *inv, float *out, hipStream_t st) {
    const dim3 block(256);
    const int width = N <= 16 ? 16 : (N <= 32 ? 32 : (N <= 64 ? 64 : (N <= 128 ? 128 : 256)));   // output columns per workgroup
    const dim3 grid((n + 31) / 32, (N + width - 1) / width);
    const uint64_t nt = static_cast<uint64_t>(n_tiles);
#define QGTC_TILED_ATT_LAUNCH(LPR, CPL) \
    hipLaunchKernelGGL((k_tiled_att_f32<LPR, CPL, BWD>), grid, block, 0, st, row_ptr, kquad, tiles, nt, n, X, N, att, m, inv, out)
    switch (width) {
        case 16: QGTC_TILED_ATT_LAUNCH(16, 1); break;
        case 32: QGTC_TILED_ATT_LAUNCH(16, 2); break;
        case 64: QGTC_TILED_ATT_LAUNCH(16, 4); break;
        case 128: QGTC_TILED_ATT_LAUNCH(32, 4); break;
        default: QGTC_TILED_ATT_LAUNCH(64, 4); break;
    }
#undef QGTC_TILED_ATT_LAUNCH
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

// the out node's row in registers up to N = 256, read again per neighbour beyond (tests/tiled_attn_model.py, ATT_GRAD_VARIANTS)
template <bool NBR_OWNS>
int tiled_att_grad(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *A,
                   const float *B, int N, const TiledAtt &att, float *out, hipStream_t st) {
    const dim3 block(256), grid((n + 31) / 32);
    const uint64_t nt = static_cast<uint64_t>(n_tiles);
    if (N <= 256)
        hipLaunchKernelGGL((k_tiled_att_grad<true, NBR_OWNS>), grid, block, 0, st, row_ptr, kquad, tiles, nt, n, A, B, N, att, out);
    else
        hipLaunchKernelGGL((k_tiled_att_grad<false, NBR_OWNS>), grid, block, 0, st, row_ptr, kquad, tiles, nt, n, A, B, N, att, out);
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

}  // namespace

int qgtc_tiledatt_f32(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *X,
                      size_t x_elems, int N, const float *att_own, const float *att_nbr, float negative_slope, int backward,
                      const float *shift, float *m, float *inv, float *out, size_t out_elems, void *stream) {
    if (backward < 0 || backward > 1) return QGTC_EINVAL;
    const float *const vec[] = {att_own, att_nbr, shift, inv, backward ? shift : m};
    const int rc = tiled_att_args_ok(row_ptr && kquad, tiles, n_tiles, n, X, x_elems, N, out, out_elems, static_cast<size_t>(N > 0 ? N : 0),
                                     negative_slope, vec);
    if (rc != QGTC_OK) return rc;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const TiledAtt att{att_own, att_nbr, shift, backward ? inv : nullptr, nullptr, negative_slope};   // the forward only writes inv
    return backward ? tiled_att_f32<true>(row_ptr, kquad, tiles, n_tiles, n, X, N, att, nullptr, nullptr, out, st)
                    : tiled_att_f32<false>(row_ptr, kquad, tiles, n_tiles, n, X, N, att, m, inv, out, st);
}

int qgtc_tiledatt_grad_f32(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *A,
                           const float *B, size_t ab_elems, int N, const float *att_own, const float *att_nbr, float negative_slope,
                           int nbr_owns, const float *m, const float *inv, const float *D, float *out, size_t out_elems, void *stream) {
    if (nbr_owns < 0 || nbr_owns > 1) return QGTC_EINVAL;
    const float *const vec[] = {B, att_own, att_nbr, m, inv, D};
    const int rc = tiled_att_args_ok(row_ptr && kquad, tiles, n_tiles, n, A, ab_elems, N, out, out_elems, 1, negative_slope, vec);
    if (rc != QGTC_OK) return rc;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const TiledAtt att{att_own, att_nbr, m, inv, D, negative_slope};
    return nbr_owns ? tiled_att_grad<true>(row_ptr, kquad, tiles, n_tiles, n, A, B, N, att, out, st)
                    : tiled_att_grad<false>(row_ptr, kquad, tiles, n_tiles, n, A, B, N, att, out, st);
}

int qgtc_rowdot_f32(const float *A, const float *B, size_t ab_elems, int n, int N, float *out, size_t out_elems, void *stream) {
    if (!A || !B || !out || n < 1 || n > (1 << 23) || N < 1) return QGTC_EINVAL;
    if (!aligned4(A) || !aligned4(B) || !aligned4(out)) return QGTC_EALIGN;
    if (ab_elems < static_cast<size_t>(n) * static_cast<size_t>(N) || out_elems < static_cast<size_t>(n)) return QGTC_ESIZE;
    hipLaunchKernelGGL(k_rowdot_f32, dim3((n + 3) / 4), dim3(256), 0, static_cast<hipStream_t>(stream), A, B, n, N, out);
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}
