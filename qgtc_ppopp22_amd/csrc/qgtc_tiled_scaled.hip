// qgtc_tiled_scaled.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): the scaled product of the
// tile-compressed adjacency, quantise(fl32(A_tiled . X) * row_scale) (the SCALED instantiations of tiled_kernels.hip.h), and the
// degrees of a tiled adjacency with their reciprocals and inverse square roots (tiled_degree_kernels.hip.h), with their launchers.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "qgtc.h"

#include "common.hip.h"
#include "bitmm_popcount.hip.h"   // requant (templates only: nothing is instantiated here)
#include "tiled_kernels.hip.h"
#include "tiled_t_kernels.hip.h"  // the butterfly of the in-degree kernel (templates only)
#include "tiled_degree_kernels.hip.h"
#include "tiled_args.hip.h"

namespace {

// the variant choice of qgtc_tiled.hip's tiled_mm
template <int MODE>
int tiled_mm_scaled(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const uint32_t *X,
                    size_t x_words, int N, int bit2, int ob, const float *row_scale, void *out, hipStream_t st) {
    const int nrb = (n + 31) / 32;
    const float maxv = std::ldexp(1.0f, ob), maxm1 = maxv - 1.0f;
    const dim3 block(256);
    const int R = N <= 16 ? 2 : (N <= 32 ? 4 : (N <= 64 ? 8 : 16));
    const dim3 grid(nrb, R == 16 ? step128(N) : 1);
    const uint64_t nt = static_cast<uint64_t>(n_tiles);
#define QGTC_TILED_LAUNCH(RR)                                                                                                          \
    hipLaunchKernelGGL((k_tiled_mm<RR, MODE, const float *>), grid, block, 0, st, row_ptr, kquad, tiles, nt, n, X,                             \
                       static_cast<uint64_t>(x_words), N, bit2, ob, maxv, maxm1, out, row_scale)
    switch (R) {
        case 2: QGTC_TILED_LAUNCH(2); break;
        case 4: QGTC_TILED_LAUNCH(4); break;
        case 8: QGTC_TILED_LAUNCH(8); break;
        default: QGTC_TILED_LAUNCH(16); break;
    }
#undef QGTC_TILED_LAUNCH
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

int degree_grid(uint64_t items) {
    const uint64_t b = (items + 255) / 256;
    return static_cast<int>(b < 8192 ? (b ? b : 1) : 8192);
}

}  // namespace

int qgtc_tiledmm2bit_scaled(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n,
                            const uint32_t *X, size_t x_words, int N, int bit2, int output_bit, const float *row_scale, uint32_t *out,
                            size_t out_words, void *stream) {
    const int rc = tiled_mm_args_ok(row_ptr, kquad, tiles, n_tiles, n, X, N, bit2, out);
    if (rc != QGTC_OK) return rc;
    if (!row_scale || !bits_ok(output_bit)) return QGTC_EINVAL;
    if (out_words < qgtc_rows_words(n, N, output_bit)) return QGTC_ESIZE;
    return tiled_mm_scaled<0>(row_ptr, kquad, tiles, n_tiles, n, X, x_words, N, bit2, output_bit, row_scale, out,
                              static_cast<hipStream_t>(stream));
}

int qgtc_tiledmm2int_scaled(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n,
                            const uint32_t *X, size_t x_words, int N, int bit2, const float *row_scale, float *out, size_t out_elems,
                            void *stream) {
    const int rc = tiled_mm_args_ok(row_ptr, kquad, tiles, n_tiles, n, X, N, bit2, out);
    if (rc != QGTC_OK) return rc;
    if (!row_scale) return QGTC_EINVAL;
    if (out_elems < static_cast<size_t>(n) * N) return QGTC_ESIZE;
    return tiled_mm_scaled<2>(row_ptr, kquad, tiles, n_tiles, n, X, x_words, N, bit2, 1, row_scale, out,
                              static_cast<hipStream_t>(stream));
}

int qgtc_tiled_degrees(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, int32_t *out_deg,
                       int32_t *in_deg, float *out_inv, float *in_inv, void *stream) {
    if (n < 1 || n > TILED_MAX_N || n_tiles < 0 || (n_tiles && (!row_ptr || !kquad || !tiles)) || (!out_deg && !in_deg) ||
        (out_inv && !out_deg) || (in_inv && !in_deg))
        return QGTC_EINVAL;
    if (tiles && !aligned16(tiles)) return QGTC_EALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint64_t nt = static_cast<uint64_t>(n_tiles);
    if (out_deg)
        hipLaunchKernelGGL(k_tiled_out_degree, dim3(degree_grid((static_cast<uint64_t>(n) + 31) / 32 * 32)), dim3(256), 0, st, row_ptr,
                           kquad, tiles, nt, n, out_deg);
    if (in_deg) {
        FILL_TRY(in_deg, 0, static_cast<size_t>(n) * sizeof(int32_t), st);
        if (nt) hipLaunchKernelGGL(k_tiled_in_degree, dim3(degree_grid(nt * 32)), dim3(256), 0, st, kquad, tiles, nt, n, in_deg);
    }
    if (out_inv || in_inv)
        hipLaunchKernelGGL(k_tiled_inv_degree, dim3(degree_grid(static_cast<uint64_t>(n))), dim3(256), 0, st, out_deg, out_inv, in_deg,
                           in_inv, n);
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

int qgtc_tiled_inv_sqrt_degree(const int32_t *deg, int n, float *out, void *stream) {
    if (!deg || !out || n < 1 || n > TILED_MAX_N) return QGTC_EINVAL;
    if ((reinterpret_cast<uintptr_t>(deg) | reinterpret_cast<uintptr_t>(out)) & 3u) return QGTC_EALIGN;
    hipLaunchKernelGGL(k_tiled_inv_sqrt_degree, dim3(degree_grid(static_cast<uint64_t>(n))), dim3(256), 0, static_cast<hipStream_t>(stream),
                       deg, out, n);
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

// the reciprocal pass of qgtc_tiled_degrees alone (k_tiled_inv_degree on one pair), for degrees that did not come from that entry
int qgtc_tiled_inv_degree(const int32_t *deg, int n, float *out, void *stream) {
    if (!deg || !out || n < 1 || n > TILED_MAX_N) return QGTC_EINVAL;
    if ((reinterpret_cast<uintptr_t>(deg) | reinterpret_cast<uintptr_t>(out)) & 3u) return QGTC_EALIGN;
    hipLaunchKernelGGL(k_tiled_inv_degree, dim3(degree_grid(static_cast<uint64_t>(n))), dim3(256), 0, static_cast<hipStream_t>(stream), deg,
                       out, static_cast<const int32_t *>(nullptr), static_cast<float *>(nullptr), n);
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}
