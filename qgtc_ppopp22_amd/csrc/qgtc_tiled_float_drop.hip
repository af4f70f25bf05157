// qgtc_tiled_float_drop.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): the float product of the
// tile-compressed adjacency under the edge-dropout mask, out = diag(row_scale) . (A_tiled masked) . diag(src_scale) . X (the
// instantiations of tiled_float_kernels.hip.h whose pack ends in the mask; include/qgtc.h, "Edge dropout"), its
// launcher, and the host-side keep test.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "qgtc.h"

#include "common.hip.h"
#include "tiled_float_kernels.hip.h"

namespace {

// the variant choice of qgtc_tiled_float.hip's tiled_mm_f32; the pack is (src_scale, mask) or (mask)
template <bool SCALED, class... Src>
int tiled_mm_f32_drop(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *X, int N,
                      const float *row_scale, float *out, hipStream_t st, Src... src) {
    const dim3 block(256);
    const int width = N <= 16 ? 16 : (N <= 32 ? 32 : (N <= 64 ? 64 : (N <= 128 ? 128 : 256)));   // output columns per workgroup
    const dim3 grid((n + 31) / 32, (N + width - 1) / width);
    const uint64_t nt = static_cast<uint64_t>(n_tiles);
#define QGTC_TILED_F32_LAUNCH(LPR, CPL)                                                                                               \
    hipLaunchKernelGGL((k_tiled_mm_f32<LPR, CPL, SCALED, Src...>), grid, block, 0, st, row_ptr, kquad, tiles, nt, n, X, N, row_scale, \
                       out, src...)
    switch (width) {
        case 16: QGTC_TILED_F32_LAUNCH(16, 1); break;
        case 32: QGTC_TILED_F32_LAUNCH(16, 2); break;
        case 64: QGTC_TILED_F32_LAUNCH(16, 4); break;
        case 128: QGTC_TILED_F32_LAUNCH(32, 4); break;
        default: QGTC_TILED_F32_LAUNCH(64, 4); break;
    }
#undef QGTC_TILED_F32_LAUNCH
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

}  // namespace

int qgtc_tiledmm_f32_drop(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *X,
                          size_t x_elems, int N, const float *row_scale, const float *src_scale, float *out, size_t out_elems,
                          uint32_t threshold, uint64_t seed, void *stream) {
    const int rc = tiled_f32_args_ok(row_ptr && kquad, tiles, n_tiles, n, X, x_elems, N, row_scale, out, out_elems, src_scale);
    if (rc != QGTC_OK) return rc;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const TiledDropView<false> mask{tiled_drop_make(threshold, seed)};
    if (src_scale)
        return row_scale ? tiled_mm_f32_drop<true>(row_ptr, kquad, tiles, n_tiles, n, X, N, row_scale, out, st, src_scale, mask)
                         : tiled_mm_f32_drop<false>(row_ptr, kquad, tiles, n_tiles, n, X, N, nullptr, out, st, src_scale, mask);
    return row_scale ? tiled_mm_f32_drop<true>(row_ptr, kquad, tiles, n_tiles, n, X, N, row_scale, out, st, mask)
                     : tiled_mm_f32_drop<false>(row_ptr, kquad, tiles, n_tiles, n, X, N, nullptr, out, st, mask);
}

// the keep test on the host: the functions the kernels run (tiled_drop.hip.h)
int qgtc_edge_kept(uint32_t i, uint32_t j, uint64_t seed, uint32_t threshold) {
    const TiledDrop d = tiled_drop_make(threshold, seed);
    return tiled_drop_test(d, tiled_drop_row_half(d, i), tiled_drop_col_half(d, j)) ? 1 : 0;
}
