// qgtc_affine_linear.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): the byte-code route of the affine
// linear layer, the C entries of include/qgtc_linear.h over the kernels of affine_linear_kernels.hip.h. Every
// entry checks, makes one launch on the caller's stream and returns: no atomics, no host read, no allocation.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "qgtc_linear.h"

#include "common.hip.h"
#include "affine_kernels.hip.h"   // aquant, range_take, range_wave, qparams_of: the quantiser and the qparams rule themselves
#include "affine_linear_kernels.hip.h"

namespace {

inline bool alin_aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
inline bool alin_codes_misaligned(const void *p, size_t ldk, int K) { return !aligned16(p) || ldk < static_cast<size_t>(K) || (ldk & 15u) != 0; }

struct AlinArgs {
    const float *x;
    int M, K;
    const float4 *qa;
    float qmax;
    const uint8_t *wt;
    size_t ldk;
    int N;
    const float4 *qb;
    int percol;
    const int32_t *col_sums;
    const float *row_scale, *bias;
    int relu;
    float *out;
};

template <int NT, bool VEC>
int alin_launch(const AlinArgs &g, hipStream_t st) {
    const int k64 = (g.K + 63) / 64 * 64;
    const int kc = k64 < alin_chunk(NT) ? k64 : alin_chunk(NT);
    const int lines = 16 * (NT < (g.N + 15) / 16 ? NT : (g.N + 15) / 16);
    const size_t lds = static_cast<size_t>(lines) * (kc + ALIN_PAD);
    const dim3 grid(static_cast<unsigned>((static_cast<long long>(g.M) + ALIN_ROWS - 1) / ALIN_ROWS), static_cast<unsigned>((g.N + 16 * NT - 1) / (16 * NT)));
    hipLaunchKernelGGL((k_affine_linear_u8<NT, VEC>), grid, dim3(64 * ALIN_WAVES), lds, st, g.x, g.M, g.K, g.qa, g.qmax, g.wt, g.ldk, g.N, g.qb,
                       g.percol, g.col_sums, g.row_scale, g.bias, g.relu, g.out, kc);
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

template <bool VEC>
int alin_pick(const AlinArgs &g, hipStream_t st) {
    const int tiles = (g.N + 15) / 16;
    if (tiles <= 1) return alin_launch<1, VEC>(g, st);
    if (tiles <= 2) return alin_launch<2, VEC>(g, st);
    if (tiles <= 4) return alin_launch<4, VEC>(g, st);
    if (tiles <= 8) return alin_launch<8, VEC>(g, st);
    return alin_launch<16, VEC>(g, st);
}

}  // namespace

int qgtc_affine_pack_weight(const float *w, int K, int N, int nbits, int per_column, float *qparams, size_t qparams_elems, uint8_t *codes_t,
                            size_t ldk, size_t codes_bytes, int32_t *col_sums, size_t sums_elems, void *stream) {
    if (!w || !qparams || !codes_t || !col_sums || K <= 0 || N <= 0 || nbits < 1 || nbits > 8 || K > QGTC_LINEAR_K_MAX) return QGTC_EINVAL;
    if (!aligned16(qparams) || alin_codes_misaligned(codes_t, ldk, K) || !alin_aligned4(w) || !alin_aligned4(col_sums)) return QGTC_EALIGN;
    const size_t groups = per_column ? static_cast<size_t>(N) : 1u;
    if (qparams_elems < 4u * groups || codes_bytes < static_cast<size_t>(N) * ldk || sums_elems < static_cast<size_t>(N)) return QGTC_ESIZE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const float qmax = static_cast<float>((1 << nbits) - 1);
    float4 *qp = reinterpret_cast<float4 *>(qparams);
    if (per_column)
        hipLaunchKernelGGL(k_affine_pack_weight<true>, dim3(N), dim3(256), 0, st, w, K, N, qmax, qp, codes_t, ldk, col_sums);
    else
        hipLaunchKernelGGL(k_affine_pack_weight<false>, dim3(N), dim3(256), 0, st, w, K, N, qmax, qp, codes_t, ldk, col_sums);
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

int qgtc_affine_linear_u8(const float *x, int M, int K, const float *qa, int a_bits, const uint8_t *codes_t, size_t ldk, size_t codes_bytes,
                          int N, const float *qb, int groups_b, const int32_t *col_sums, const float *row_scale, const float *bias,
                          int relu, float *out, size_t out_elems, void *stream) {
    if (!x || !qa || !codes_t || !qb || !col_sums || !out || M <= 0 || K <= 0 || N <= 0 || a_bits < 1 || a_bits > 8 ||
        (groups_b != 1 && groups_b != N) || K > QGTC_LINEAR_K_MAX)
        return QGTC_EINVAL;
    if (!aligned16(qa) || !aligned16(qb) || alin_codes_misaligned(codes_t, ldk, K) || !alin_aligned4(x) || !alin_aligned4(col_sums) ||
        !alin_aligned4(row_scale) || !alin_aligned4(bias) || !alin_aligned4(out))
        return QGTC_EALIGN;
    if (codes_bytes < static_cast<size_t>(N) * ldk || out_elems < static_cast<size_t>(M) * static_cast<size_t>(N)) return QGTC_ESIZE;
    const AlinArgs g{x, M, K, reinterpret_cast<const float4 *>(qa), static_cast<float>((1 << a_bits) - 1), codes_t, ldk, N,
                     reinterpret_cast<const float4 *>(qb), groups_b == N && N > 1 ? 1 : 0, col_sums, row_scale, bias, relu ? 1 : 0, out};
    hipStream_t st = static_cast<hipStream_t>(stream);
    return (K & 3) == 0 && aligned16(x) ? alin_pick<true>(g, st) : alin_pick<false>(g, st);
}
