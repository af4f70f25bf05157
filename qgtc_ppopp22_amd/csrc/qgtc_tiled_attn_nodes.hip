// qgtc_tiled_attn_nodes.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): the softmax-weighted sum over
// the neighbours in nbr_mask, of the rows in row_mask of the tile-compressed adjacency, and its gradients on this view (the
// instantiations of tiled_attn_kernels.hip.h with the node masks; include/qgtc.h, "Node masks"), and their
// launchers. `shift` of the forward must be the MASKED maximum (qgtc_tiledmax_f32_nodes with the same masks).
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

using Mask = TiledNodes;

// the variant choices of qgtc_tiled_attn.hip
template <bool BWD>
int tiled_att_f32_nodes(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *X, int N,
                       const TiledAtt &att, float *m, float *inv, float *out, const Mask &mask, hipStream_t st) {
    const dim3 block(256);
    const int width = N <= 16 ? 16 : (N <= 32 ? 32 : (N <= 64 ? 64 : (N <= 128 ? 128 : 256)));   // output columns per workgroup
    const dim3 grid((n + 31) / 32, (N + width - 1) / width);
    const uint64_t nt = static_cast<uint64_t>(n_tiles);
#define QGTC_TILED_ATT_LAUNCH(LPR, CPL)                                                                                             \
    hipLaunchKernelGGL((k_tiled_att_f32<LPR, CPL, BWD, Mask>), grid, block, 0, st, row_ptr, kquad, tiles, nt, n, X, N, att, m, inv, \
                       out, mask)
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

template <bool NBR_OWNS>
int tiled_att_grad_nodes(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *A,
                        const float *B, int N, const TiledAtt &att, float *out, const Mask &mask, hipStream_t st) {
    const dim3 block(256), grid((n + 31) / 32);
    const uint64_t nt = static_cast<uint64_t>(n_tiles);
    if (N <= 256)
        hipLaunchKernelGGL((k_tiled_att_grad<true, NBR_OWNS, Mask>), grid, block, 0, st, row_ptr, kquad, tiles, nt, n, A, B, N, att, out,
                           mask);
    else
        hipLaunchKernelGGL((k_tiled_att_grad<false, NBR_OWNS, Mask>), grid, block, 0, st, row_ptr, kquad, tiles, nt, n, A, B, N, att, out,
                           mask);
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

}  // namespace

int qgtc_tiledatt_f32_nodes(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *X,
                           size_t x_elems, int N, const float *att_own, const float *att_nbr, float negative_slope, int backward,
                           const float *shift, float *m, float *inv, float *out, size_t out_elems, const uint32_t *row_mask, const uint32_t *nbr_mask, size_t mask_words,
                           void *stream) {
    if (backward < 0 || backward > 1) return QGTC_EINVAL;
    const float *const vec[] = {att_own, att_nbr, shift, inv, backward ? shift : m};
    int rc = tiled_att_args_ok(row_ptr && kquad, tiles, n_tiles, n, X, x_elems, N, out, out_elems, static_cast<size_t>(N > 0 ? N : 0),
                                     negative_slope, vec);
    if (rc == QGTC_OK) rc = tiled_nodes_args_ok(row_mask, nbr_mask, mask_words, n);
    if (rc != QGTC_OK) return rc;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const TiledAtt att{att_own, att_nbr, shift, backward ? inv : nullptr, nullptr, negative_slope};   // the forward only writes inv
    const Mask mask{row_mask, nbr_mask};
    return backward ? tiled_att_f32_nodes<true>(row_ptr, kquad, tiles, n_tiles, n, X, N, att, nullptr, nullptr, out, mask, st)
                    : tiled_att_f32_nodes<false>(row_ptr, kquad, tiles, n_tiles, n, X, N, att, m, inv, out, mask, st);
}

int qgtc_tiledatt_grad_f32_nodes(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n,
                                const float *A, const float *B, size_t ab_elems, int N, const float *att_own, const float *att_nbr,
                                float negative_slope, int nbr_owns, const float *m, const float *inv, const float *D, float *out,
                                size_t out_elems, const uint32_t *row_mask, const uint32_t *nbr_mask, size_t mask_words, void *stream) {
    if (nbr_owns < 0 || nbr_owns > 1) return QGTC_EINVAL;
    const float *const vec[] = {B, att_own, att_nbr, m, inv, D};
    int rc = tiled_att_args_ok(row_ptr && kquad, tiles, n_tiles, n, A, ab_elems, N, out, out_elems, 1, negative_slope, vec);
    if (rc == QGTC_OK) rc = tiled_nodes_args_ok(row_mask, nbr_mask, mask_words, n);
    if (rc != QGTC_OK) return rc;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const TiledAtt att{att_own, att_nbr, m, inv, D, negative_slope};
    const Mask mask{row_mask, nbr_mask};
    return nbr_owns ? tiled_att_grad_nodes<true>(row_ptr, kquad, tiles, n_tiles, n, A, B, N, att, out, mask, st)
                    : tiled_att_grad_nodes<false>(row_ptr, kquad, tiles, n_tiles, n, A, B, N, att, out, mask, st);
}
