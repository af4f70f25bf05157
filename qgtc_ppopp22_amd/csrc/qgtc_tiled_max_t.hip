// qgtc_tiled_max_t.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): the element-wise maximum / minimum
// over the neighbours of every column of the tile-compressed adjacency with the winner's id, and the select that is its gradient on
// this view (tiled_max_t_kernels.hip.h), and their launcher.
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

// columns per lane by N (16 lanes per output row). The extremum keeps two words of state a column and stops at 32 columns a workgroup;
// the select keeps one and goes to 64 like the float product (tests/tiled_max_model.py, MAX_TRANSPOSED_VARIANTS and
// SELECT_TRANSPOSED_VARIANTS, state the same choice)
template <class Red>
int tiled_red_f32_t(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles, int64_t n_tiles,
                    int n, int N, const Red &red, hipStream_t st) {
    const dim3 block(256);
    constexpr int widest = Red::WORDS == 2 ? 32 : 64;
    const int width = N <= 16 ? 16 : (N <= 32 ? 32 : widest);
    const dim3 grid(step128(n), (N + width - 1) / width);
    const uint64_t nt = static_cast<uint64_t>(n_tiles);
#define QGTC_TILED_RED_T_LAUNCH(CPL) \
    hipLaunchKernelGGL((k_tiled_red_f32_t<16, CPL, Red>), grid, block, 0, st, col_ptr, col_tile, col_rb, tiles, nt, n, N, red)
    switch (width) {
        case 16: QGTC_TILED_RED_T_LAUNCH(1); break;
        case 32: QGTC_TILED_RED_T_LAUNCH(2); break;
        default:
            if constexpr (Red::WORDS == 1) QGTC_TILED_RED_T_LAUNCH(4);
            break;
    }
#undef QGTC_TILED_RED_T_LAUNCH
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

}  // namespace

int qgtc_tiledmax_f32_t(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles, int64_t n_tiles,
                        int n, const float *X, size_t x_elems, int N, int op, float *out, size_t out_elems, int32_t *arg,
                        size_t arg_elems, void *stream) {
    const int rc = tiled_red_args_ok(col_ptr && col_tile && col_rb, tiles, n_tiles, n, X, x_elems, N, out, out_elems, arg, arg_elems,
                                     false, op);
    if (rc != QGTC_OK) return rc;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    return op ? tiled_red_f32_t(col_ptr, col_tile, col_rb, tiles, n_tiles, n, N, TiledExtremum<true>{X, out, arg}, st)
              : tiled_red_f32_t(col_ptr, col_tile, col_rb, tiles, n_tiles, n, N, TiledExtremum<false>{X, out, arg}, st);
}

int qgtc_tiledsel_f32_t(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles, int64_t n_tiles,
                        int n, const float *dY, size_t dy_elems, int N, const int32_t *arg, size_t arg_elems, float *out,
                        size_t out_elems, void *stream) {
    const int rc = tiled_red_args_ok(col_ptr && col_tile && col_rb, tiles, n_tiles, n, dY, dy_elems, N, out, out_elems, arg, arg_elems,
                                     true, 0);
    if (rc != QGTC_OK) return rc;
    return tiled_red_f32_t(col_ptr, col_tile, col_rb, tiles, n_tiles, n, N, TiledSelect{dY, arg, out}, static_cast<hipStream_t>(stream));
}
