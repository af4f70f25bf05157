// qgtc_tiled_max_nodes.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): the element-wise maximum / minimum
// over the neighbours in nbr_mask of the rows in row_mask, on both views of the tile-compressed adjacency (the instantiations of
// tiled_max_kernels.hip.h and tiled_max_t_kernels.hip.h with the node masks; include/qgtc.h, "Node masks"), and
// their launchers. The select needs no mask: arg names participating neighbours only, and a row outside row_mask has arg -1.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "qgtc.h"

#include "common.hip.h"
#include "bitmm_popcount.hip.h"   // requant, for tiled_t_kernels.hip.h (templates only: nothing is instantiated here)
#include "tiled_t_kernels.hip.h"  // the in-register bit transpose
#include "tiled_float_kernels.hip.h"
#include "tiled_max_kernels.hip.h"
#include "tiled_max_t_kernels.hip.h"

namespace {

// the variant choices of qgtc_tiled_max.hip and qgtc_tiled_max_t.hip
template <class Red>
int tiled_red_f32_nodes(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, int N, const Red &red,
                       const TiledNodes &mask, hipStream_t st) {
    const dim3 block(256);
    const int width = N <= 16 ? 16 : (N <= 32 ? 32 : (N <= 64 ? 64 : (N <= 128 ? 128 : 256)));   // output columns per workgroup
    const dim3 grid((n + 31) / 32, (N + width - 1) / width);
    const uint64_t nt = static_cast<uint64_t>(n_tiles);
#define QGTC_TILED_RED_LAUNCH(LPR, CPL)                                                                                             \
    hipLaunchKernelGGL((k_tiled_red_f32<LPR, CPL, Red, TiledNodes>), grid, block, 0, st, row_ptr, kquad, tiles, nt, n, N, \
                       red, mask)
    switch (width) {
        case 16: QGTC_TILED_RED_LAUNCH(16, 1); break;
        case 32: QGTC_TILED_RED_LAUNCH(16, 2); break;
        case 64: QGTC_TILED_RED_LAUNCH(16, 4); break;
        case 128: QGTC_TILED_RED_LAUNCH(32, 4); break;
        default: QGTC_TILED_RED_LAUNCH(64, 4); break;
    }
#undef QGTC_TILED_RED_LAUNCH
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

template <class Red>
int tiled_red_f32_t_nodes(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles, int64_t n_tiles,
                         int n, int N, const Red &red, const TiledNodes &mask, hipStream_t st) {
    static_assert(Red::WORDS == 2, "the extremum: two words of state a column, 32 columns a workgroup");
    const dim3 block(256);
    const int width = N <= 16 ? 16 : 32;
    const dim3 grid(step128(n), (N + width - 1) / width);
    const uint64_t nt = static_cast<uint64_t>(n_tiles);
    if (width == 16)
        hipLaunchKernelGGL((k_tiled_red_f32_t<16, 1, Red, TiledNodes>), grid, block, 0, st, col_ptr, col_tile, col_rb, tiles, nt,
                           n, N, red, mask);
    else
        hipLaunchKernelGGL((k_tiled_red_f32_t<16, 2, Red, TiledNodes>), grid, block, 0, st, col_ptr, col_tile, col_rb, tiles, nt,
                           n, N, red, mask);
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

}  // namespace

int qgtc_tiledmax_f32_nodes(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *X,
                           size_t x_elems, int N, int op, float *out, size_t out_elems, int32_t *arg, size_t arg_elems,
                           const uint32_t *row_mask, const uint32_t *nbr_mask, size_t mask_words, void *stream) {
    int rc = tiled_red_args_ok(row_ptr && kquad, tiles, n_tiles, n, X, x_elems, N, out, out_elems, arg, arg_elems, false, op);
    if (rc == QGTC_OK) rc = tiled_nodes_args_ok(row_mask, nbr_mask, mask_words, n);
    if (rc != QGTC_OK) return rc;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const TiledNodes mask{row_mask, nbr_mask};
    return op ? tiled_red_f32_nodes(row_ptr, kquad, tiles, n_tiles, n, N, TiledExtremum<true>{X, out, arg}, mask, st)
              : tiled_red_f32_nodes(row_ptr, kquad, tiles, n_tiles, n, N, TiledExtremum<false>{X, out, arg}, mask, st);
}

int qgtc_tiledmax_f32_t_nodes(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                             int64_t n_tiles, int n, const float *X, size_t x_elems, int N, int op, float *out, size_t out_elems,
                             int32_t *arg, size_t arg_elems, const uint32_t *row_mask, const uint32_t *nbr_mask, size_t mask_words,
                             void *stream) {
    int rc = tiled_red_args_ok(col_ptr && col_tile && col_rb, tiles, n_tiles, n, X, x_elems, N, out, out_elems, arg, arg_elems, false, op);
    if (rc == QGTC_OK) rc = tiled_nodes_args_ok(row_mask, nbr_mask, mask_words, n);
    if (rc != QGTC_OK) return rc;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const TiledNodes mask{row_mask, nbr_mask};
    return op ? tiled_red_f32_t_nodes(col_ptr, col_tile, col_rb, tiles, n_tiles, n, N, TiledExtremum<true>{X, out, arg}, mask, st)
              : tiled_red_f32_t_nodes(col_ptr, col_tile, col_rb, tiles, n_tiles, n, N, TiledExtremum<false>{X, out, arg}, mask, st);
}
