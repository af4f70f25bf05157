// qgtc_tiled_float_t_nodes.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): the transposed float
// product of the tile-compressed adjacency under node masks, out = diag(row_scale) . (A_tiled^T restricted to row_mask x nbr_mask) .
// diag(src_scale) . X (the instantiations of tiled_float_t_kernels.hip.h whose pack ends in the masks; include/qgtc.h, "Node masks";
// DESIGN.md section 6.15e), and its launcher. The masks are relative to the view: row_mask names output rows (A's columns).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "qgtc.h"

#include "common.hip.h"
#include "bitmm_popcount.hip.h"   // requant, for tiled_t_kernels.hip.h (templates only: nothing is instantiated here)
#include "tiled_t_kernels.hip.h"  // the in-register bit transpose
#include "tiled_float_kernels.hip.h"
#include "tiled_float_t_kernels.hip.h"

namespace {

// the variant choice of qgtc_tiled_float_t.hip's tiled_mm_f32_t; the pack is (src_scale, masks) or (masks)
template <bool SCALED, class... Src>
int tiled_mm_f32_t_nodes(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles, int64_t n_tiles,
                        int n, const float *X, int N, const float *row_scale, float *out, hipStream_t st, Src... src) {
    const dim3 block(256);
    const int width = N <= 16 ? 16 : (N <= 32 ? 32 : 64);
    const dim3 grid(step128(n), (N + width - 1) / width);
    const uint64_t nt = static_cast<uint64_t>(n_tiles);
#define QGTC_TILED_F32_T_LAUNCH(CPL)                                                                                                 \
    hipLaunchKernelGGL((k_tiled_mm_f32_t<16, CPL, SCALED, Src...>), grid, block, 0, st, col_ptr, col_tile, col_rb, tiles, nt, n, X, N, \
                       row_scale, out, src...)
    switch (width) {
        case 16: QGTC_TILED_F32_T_LAUNCH(1); break;
        case 32: QGTC_TILED_F32_T_LAUNCH(2); break;
        default: QGTC_TILED_F32_T_LAUNCH(4); break;
    }
#undef QGTC_TILED_F32_T_LAUNCH
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

}  // namespace

int qgtc_tiledmm_f32_t_nodes(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                             int64_t n_tiles, int n, const float *X, size_t x_elems, int N, const float *row_scale,
                             const float *src_scale, float *out, size_t out_elems, const uint32_t *row_mask, const uint32_t *nbr_mask,
                             size_t mask_words, void *stream) {
    int rc = tiled_f32_args_ok(col_ptr && col_tile && col_rb, tiles, n_tiles, n, X, x_elems, N, row_scale, out, out_elems, src_scale);
    if (rc == QGTC_OK) rc = tiled_nodes_args_ok(row_mask, nbr_mask, mask_words, n);
    if (rc != QGTC_OK) return rc;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const TiledNodes mask{row_mask, nbr_mask};
    if (src_scale)
        return row_scale ? tiled_mm_f32_t_nodes<true>(col_ptr, col_tile, col_rb, tiles, n_tiles, n, X, N, row_scale, out, st, src_scale, mask)
                         : tiled_mm_f32_t_nodes<false>(col_ptr, col_tile, col_rb, tiles, n_tiles, n, X, N, nullptr, out, st, src_scale, mask);
    return row_scale ? tiled_mm_f32_t_nodes<true>(col_ptr, col_tile, col_rb, tiles, n_tiles, n, X, N, row_scale, out, st, mask)
                     : tiled_mm_f32_t_nodes<false>(col_ptr, col_tile, col_rb, tiles, n_tiles, n, X, N, nullptr, out, st, mask);
}
