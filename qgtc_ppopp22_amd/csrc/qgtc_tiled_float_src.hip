// qgtc_tiled_float_src.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): the float product of the
// tile-compressed adjacency with a scale on the SOURCE row, out = diag(row_scale) . A_tiled . diag(src_scale) . X (the instantiations
// of tiled_float_kernels.hip.h with a source scale), and its launcher.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "qgtc.h"

#include "common.hip.h"
#include "tiled_float_kernels.hip.h"

namespace {

// the variant choice of qgtc_tiled_float.hip's tiled_mm_f32
template <bool SCALED>
int tiled_mm_f32_src(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *X, int N,
                     const float *row_scale, const float *src_scale, float *out, hipStream_t st) {
    const dim3 block(256);
    const int width = N <= 16 ? 16 : (N <= 32 ? 32 : (N <= 64 ? 64 : (N <= 128 ? 128 : 256)));   // output columns per workgroup
    const dim3 grid((n + 31) / 32, (N + width - 1) / width);
    const uint64_t nt = static_cast<uint64_t>(n_tiles);
#define QGTC_TILED_F32_LAUNCH(LPR, CPL)                                                                                                \
    hipLaunchKernelGGL((k_tiled_mm_f32<LPR, CPL, SCALED, const float *>), grid, block, 0, st, row_ptr, kquad, tiles, nt, n, X, N,       \
                       row_scale, out, src_scale)
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

int qgtc_tiledmm_f32_src(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *X,
                         size_t x_elems, int N, const float *row_scale, const float *src_scale, float *out, size_t out_elems,
                         void *stream) {
    if (!src_scale) return qgtc_tiledmm_f32(row_ptr, kquad, tiles, n_tiles, n, X, x_elems, N, row_scale, out, out_elems, stream);
    const int rc = tiled_f32_args_ok(row_ptr && kquad, tiles, n_tiles, n, X, x_elems, N, row_scale, out, out_elems, src_scale);
    if (rc != QGTC_OK) return rc;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    return row_scale ? tiled_mm_f32_src<true>(row_ptr, kquad, tiles, n_tiles, n, X, N, row_scale, src_scale, out, st)
                     : tiled_mm_f32_src<false>(row_ptr, kquad, tiles, n_tiles, n, X, N, nullptr, src_scale, out, st);
}
