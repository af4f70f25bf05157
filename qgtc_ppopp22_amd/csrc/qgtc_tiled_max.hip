// qgtc_tiled_max.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): the element-wise maximum / minimum
// over the neighbours of every row of the tile-compressed adjacency with the winner's id, and the select that is its gradient on this
// view (tiled_max_kernels.hip.h), and their launcher.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "qgtc.h"

#include "common.hip.h"
#include "tiled_float_kernels.hip.h"
#include "tiled_max_kernels.hip.h"

namespace {

// lanes per output row and columns per lane by N: the float product's choice (qgtc_tiled_float.hip; tests/tiled_max_model.py,
// MAX_FORWARD_VARIANTS, states the same)
template <class Red>
int tiled_red_f32(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, int N, const Red &red,
                  hipStream_t st) {
    const dim3 block(256);
    const int width = N <= 16 ? 16 : (N <= 32 ? 32 : (N <= 64 ? 64 : (N <= 128 ? 128 : 256)));   // output columns per workgroup
    const dim3 grid((n + 31) / 32, (N + width - 1) / width);
    const uint64_t nt = static_cast<uint64_t>(n_tiles);
#define QGTC_TILED_RED_LAUNCH(LPR, CPL) \
    hipLaunchKernelGGL((k_tiled_red_f32<LPR, CPL, Red>), grid, block, 0, st, row_ptr, kquad, tiles, nt, n, N, red)
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

}  // namespace

int qgtc_tiledmax_f32(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *X,
                      size_t x_elems, int N, int op, float *out, size_t out_elems, int32_t *arg, size_t arg_elems, void *stream) {
    const int rc = tiled_red_args_ok(row_ptr && kquad, tiles, n_tiles, n, X, x_elems, N, out, out_elems, arg, arg_elems, false, op);
    if (rc != QGTC_OK) return rc;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    return op ? tiled_red_f32(row_ptr, kquad, tiles, n_tiles, n, N, TiledExtremum<true>{X, out, arg}, st)
              : tiled_red_f32(row_ptr, kquad, tiles, n_tiles, n, N, TiledExtremum<false>{X, out, arg}, st);
}

int qgtc_tiledsel_f32(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *dY,
                      size_t dy_elems, int N, const int32_t *arg, size_t arg_elems, float *out, size_t out_elems, void *stream) {
    const int rc = tiled_red_args_ok(row_ptr && kquad, tiles, n_tiles, n, dY, dy_elems, N, out, out_elems, arg, arg_elems, true, 0);
    if (rc != QGTC_OK) return rc;
    return tiled_red_f32(row_ptr, kquad, tiles, n_tiles, n, N, TiledSelect{dY, arg, out}, static_cast<hipStream_t>(stream));
}
