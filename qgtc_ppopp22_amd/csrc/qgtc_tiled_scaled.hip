// qgtc_tiled_scaled.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): the scaled product of the
// tile-compressed adjacency, quantise(fl32(A_tiled . X) * row_scale): the entries that hand tiled_kernels.hip.h's launcher a row_scale, and
// with them the kernel's instantiations with that pack; and the degrees of a tiled adjacency with their reciprocals and inverse square
// roots (tiled_degree_kernels.hip.h), with their launchers.
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

int qgtc_tiledmm2bit_scaled(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n,
                            const uint32_t *X, size_t x_words, int N, int bit2, int output_bit, const float *row_scale, uint32_t *out,
                            size_t out_words, void *stream) {
    const TiledRowIndex ix{row_ptr, kquad};
    return tiled_mm_entry<0>(ix, tiles, n_tiles, n, X, x_words, N, bit2, output_bit, out, out_words, stream, row_scale);
}

int qgtc_tiledmm2int_scaled(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n,
                            const uint32_t *X, size_t x_words, int N, int bit2, const float *row_scale, float *out, size_t out_elems,
                            void *stream) {
    const TiledRowIndex ix{row_ptr, kquad};
    return tiled_mm_entry<2>(ix, tiles, n_tiles, n, X, x_words, N, bit2, 1, out, out_elems, stream, row_scale);
}

int qgtc_tiled_degrees(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, int32_t *out_deg,
                       int32_t *in_deg, float *out_inv, float *in_inv, void *stream) {
    if (tiled_adj_malformed(TiledRowIndex{row_ptr, kquad}.ok(), tiles, n_tiles, n) || (!out_deg && !in_deg) || (out_inv && !out_deg) ||
        (in_inv && !in_deg))
        return QGTC_EINVAL;
    if (tiled_adj_misaligned(tiles)) return QGTC_EALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint64_t nt = static_cast<uint64_t>(n_tiles);
    if (out_deg)
        hipLaunchKernelGGL(k_tiled_out_degree, dim3(tiled_grid_1d((static_cast<uint64_t>(n) + 31) / 32 * 32)), dim3(256), 0, st, row_ptr,
                           kquad, tiles, nt, n, out_deg);
    if (in_deg) {
        FILL_TRY(in_deg, 0, static_cast<size_t>(n) * sizeof(int32_t), st);
        if (nt) hipLaunchKernelGGL(k_tiled_in_degree, dim3(tiled_grid_1d(nt * 32)), dim3(256), 0, st, kquad, tiles, nt, n, in_deg);
    }
    if (out_inv || in_inv)
        hipLaunchKernelGGL(k_tiled_inv_degree, dim3(tiled_grid_1d(static_cast<uint64_t>(n))), dim3(256), 0, st, out_deg, out_inv, in_deg,
                           in_inv, n);
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

int qgtc_tiled_inv_sqrt_degree(const int32_t *deg, int n, float *out, void *stream) {
    if (!deg || !out || n < 1 || n > TILED_MAX_N) return QGTC_EINVAL;
    if ((reinterpret_cast<uintptr_t>(deg) | reinterpret_cast<uintptr_t>(out)) & 3u) return QGTC_EALIGN;
    hipLaunchKernelGGL(k_tiled_inv_sqrt_degree, dim3(tiled_grid_1d(static_cast<uint64_t>(n))), dim3(256), 0, static_cast<hipStream_t>(stream),
                       deg, out, n);
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

// the reciprocal pass of qgtc_tiled_degrees alone (k_tiled_inv_degree on one pair), for degrees that did not come from that entry
int qgtc_tiled_inv_degree(const int32_t *deg, int n, float *out, void *stream) {
    if (!deg || !out || n < 1 || n > TILED_MAX_N) return QGTC_EINVAL;
    if ((reinterpret_cast<uintptr_t>(deg) | reinterpret_cast<uintptr_t>(out)) & 3u) return QGTC_EALIGN;
    hipLaunchKernelGGL(k_tiled_inv_degree, dim3(tiled_grid_1d(static_cast<uint64_t>(n))), dim3(256), 0, static_cast<hipStream_t>(stream), deg,
                       out, static_cast<const int32_t *>(nullptr), static_cast<float *>(nullptr), n);
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}
