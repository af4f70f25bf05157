// qgtc_tiled_float.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): the product of the tile-compressed
// adjacency with a float32 right operand, out = A_tiled . X with an optional per-row scale (tiled_float_kernels.hip.h), and its launcher.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "qgtc.h"

#include "common.hip.h"
#include "tiled_float_kernels.hip.h"

namespace {

// lanes per output row and columns per lane by N (tests/tiled_float_model.py, FLOAT_FORWARD_VARIANTS, states the same choice)
template <bool SCALED>
int tiled_mm_f32(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *X, int N,
                 const float *row_scale, float *out, hipStream_t st) {
    const dim3 block(256);
    const int width = N <= 16 ? 16 : (N <= 32 ? 32 : (N <= 64 ? 64 : (N <= 128 ? 128 : 256)));   // output columns per workgroup
    const dim3 grid((n + 31) / 32, (N + width - 1) / width);
    const uint64_t nt = static_cast<uint64_t>(n_tiles);
#define QGTC_TILED_F32_LAUNCH(LPR, CPL) \
    hipLaunchKernelGGL((k_tiled_mm_f32<LPR, CPL, SCALED>), grid, block, 0, st, row_ptr, kquad, tiles, nt, n, X, N, row_scale, out)
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

int qgtc_tiledmm_f32(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *X,
                     size_t x_elems, int N, const float *row_scale, float *out, size_t out_elems, void *stream) {
    const int rc = tiled_f32_args_ok(row_ptr && kquad, tiles, n_tiles, n, X, x_elems, N, row_scale, out, out_elems);
    if (rc != QGTC_OK) return rc;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    return row_scale ? tiled_mm_f32<true>(row_ptr, kquad, tiles, n_tiles, n, X, N, row_scale, out, st)
                     : tiled_mm_f32<false>(row_ptr, kquad, tiles, n_tiles, n, X, N, nullptr, out, st);
}
