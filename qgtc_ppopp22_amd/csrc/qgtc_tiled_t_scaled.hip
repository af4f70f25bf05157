// qgtc_tiled_t_scaled.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): the scaled transposed product
// of the tile-compressed adjacency, quantise(fl32(A_tiled^T . X) * row_scale) (the SCALED instantiations of tiled_t_kernels.hip.h),
// and its launchers.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "qgtc.h"

#include "common.hip.h"
#include "bitmm_popcount.hip.h"   // requant (templates only: nothing is instantiated here)
#include "tiled_t_kernels.hip.h"
#include "tiled_args.hip.h"

namespace {

// the variant choice of qgtc_tiled_t.hip's tiled_mm_t
template <int MODE>
int tiled_mm_t_scaled(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles, int64_t n_tiles,
                      int n, const uint32_t *X, size_t x_words, int N, int bit2, int ob, const float *row_scale, void *out,
                      hipStream_t st) {
    const float maxv = std::ldexp(1.0f, ob), maxm1 = maxv - 1.0f;
    const dim3 block(256);
    const int R = N <= 16 ? 8 : (N <= 32 ? 16 : (N <= 64 ? 32 : 64));
    const dim3 grid(step128(n), R == 64 ? step128(N) : 1);
    const uint64_t nt = static_cast<uint64_t>(n_tiles);
#define QGTC_TILED_T_LAUNCH(RR)                                                                                                        \
    hipLaunchKernelGGL((k_tiled_mm_t<RR, MODE, const float *>), grid, block, 0, st, col_ptr, col_tile, col_rb, tiles, nt, n, X,                \
                       static_cast<uint64_t>(x_words), N, bit2, ob, maxv, maxm1, out, row_scale)
    switch (R) {
        case 8: QGTC_TILED_T_LAUNCH(8); break;
        case 16: QGTC_TILED_T_LAUNCH(16); break;
        case 32: QGTC_TILED_T_LAUNCH(32); break;
        default: QGTC_TILED_T_LAUNCH(64); break;
    }
#undef QGTC_TILED_T_LAUNCH
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

}  // namespace

int qgtc_tiledmm2bit_t_scaled(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                              int64_t n_tiles, int n, const uint32_t *X, size_t x_words, int N, int bit2, int output_bit,
                              const float *row_scale, uint32_t *out, size_t out_words, void *stream) {
    const int rc = tiled_mm_t_args_ok(col_ptr, col_tile, col_rb, tiles, n_tiles, n, X, N, bit2, out);
    if (rc != QGTC_OK) return rc;
    if (!row_scale || !bits_ok(output_bit)) return QGTC_EINVAL;
    if (out_words < qgtc_rows_words(n, N, output_bit)) return QGTC_ESIZE;
    return tiled_mm_t_scaled<0>(col_ptr, col_tile, col_rb, tiles, n_tiles, n, X, x_words, N, bit2, output_bit, row_scale, out,
                                static_cast<hipStream_t>(stream));
}

int qgtc_tiledmm2int_t_scaled(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                              int64_t n_tiles, int n, const uint32_t *X, size_t x_words, int N, int bit2, const float *row_scale,
                              float *out, size_t out_elems, void *stream) {
    const int rc = tiled_mm_t_args_ok(col_ptr, col_tile, col_rb, tiles, n_tiles, n, X, N, bit2, out);
    if (rc != QGTC_OK) return rc;
    if (!row_scale) return QGTC_EINVAL;
    if (out_elems < static_cast<size_t>(n) * N) return QGTC_ESIZE;
    return tiled_mm_t_scaled<2>(col_ptr, col_tile, col_rb, tiles, n_tiles, n, X, x_words, N, bit2, 1, row_scale, out,
                                static_cast<hipStream_t>(stream));
}
