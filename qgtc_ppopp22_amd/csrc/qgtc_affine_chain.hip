// qgtc_affine_chain.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): the static affine chain, the C
// entries of include/qgtc_chain.h - the byte-code product with uint8 codes on either side over the kernels of
// affine_chain_kernels.hip.h, and the re-quantising walks on both views of the tiled adjacency over the third mode of
// tiled_codes_kernels.hip.h. Every entry checks, makes one launch on the caller's stream and returns: no atomics, no host read, no
// allocation.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "qgtc_chain.h"

#include "common.hip.h"
#include "affine_kernels.hip.h"          // aquant: the quantiser itself
#include "affine_linear_kernels.hip.h"   // the split, the chunk rule and the constants of the byte-code product
#include "affine_chain_kernels.hip.h"
#include "bitmm_popcount.hip.h"          // requant, for tiled_t_kernels.hip.h (templates only: nothing is instantiated here)
#include "tiled_codes_kernels.hip.h"

namespace {

struct ChainLeft {
    const float *x;
    const uint8_t *xq;
    size_t ldx;
    int M, K;
    const float4 *qa;
    float qmax;
};

// IN: 0 float32, a float at a time; 1 float32, 16 bytes at a time; 2 codes, a dword at a time; 3 codes, 16 bytes at a time
template <int NT, int IN, bool OUTQ>
int chain_launch(const ChainLeft &l, const AlinRight &w, const AlinOut &o, hipStream_t st) {
    const int k64 = (l.K + 63) / 64 * 64;
    const int kc = k64 < alin_chunk(NT) ? k64 : alin_chunk(NT);
    const int lines = 16 * (NT < (w.N + 15) / 16 ? NT : (w.N + 15) / 16);
    const size_t lds = static_cast<size_t>(lines) * (kc + ALIN_PAD);
    const dim3 grid(static_cast<unsigned>((static_cast<long long>(l.M) + ALIN_ROWS - 1) / ALIN_ROWS),
                    static_cast<unsigned>((w.N + 16 * NT - 1) / (16 * NT)));
    if constexpr (IN >= 2) {
        hipLaunchKernelGGL((k_affine_linear_q8<NT, IN == 3, OUTQ>), grid, dim3(64 * ALIN_WAVES), lds, st, l.xq, l.ldx, l.M, l.K, l.qa, w, o, kc);
    } else {
        static_assert(OUTQ, "float in, float out is k_affine_linear_u8");
        hipLaunchKernelGGL((k_affine_linear_u8q<NT, IN == 1>), grid, dim3(64 * ALIN_WAVES), lds, st, l.x, l.M, l.K, l.qa, l.qmax, w, o, kc);
    }
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

template <int IN, bool OUTQ>
int chain_pick(const ChainLeft &l, const AlinRight &w, const AlinOut &o, hipStream_t st) {
    const int tiles = (w.N + 15) / 16;
    if (tiles <= 1) return chain_launch<1, IN, OUTQ>(l, w, o, st);
    if (tiles <= 2) return chain_launch<2, IN, OUTQ>(l, w, o, st);
    if (tiles <= 4) return chain_launch<4, IN, OUTQ>(l, w, o, st);
    if (tiles <= 8) return chain_launch<8, IN, OUTQ>(l, w, o, st);
    return chain_launch<16, IN, OUTQ>(l, w, o, st);
}

}  // namespace

int qgtc_affine_linear_chain(const float *x, const uint8_t *xq, size_t ldx, size_t xq_bytes, int M, int K, const float *qa, int a_bits,
                             const uint8_t *codes_t, size_t ldk, size_t codes_bytes, int N, const float *qb, int groups_b,
                             const int32_t *col_sums, const float *row_scale, const float *bias, int relu, float *out, size_t out_elems,
                             uint8_t *outq, size_t ldo, size_t outq_bytes, const float *out_qp, int out_bits, void *stream) {
    const CodesDest d{out, out_elems, outq, ldo, outq_bytes, out_qp, out_bits};
    if (!qa || !codes_t || !qb || !col_sums || M <= 0 || K <= 0 || N <= 0 || a_bits < 1 || a_bits > 8 || (groups_b != 1 && groups_b != N) ||
        K > QGTC_LINEAR_K_MAX || (x != nullptr) == (xq != nullptr) || (x && out) || codes_dest_invalid(d))
        return QGTC_EINVAL;
    const bool w_off = !aligned16(codes_t) || ldk < static_cast<size_t>(K) || (ldk & 15u) != 0;
    if (!aligned16(qa) || !aligned16(qb) || w_off || !codes_aligned4(x) || !codes_aligned4(col_sums) || !codes_aligned4(row_scale) ||
        !codes_aligned4(bias) || (xq && codes_matrix_misaligned(xq, ldx, K)) || codes_dest_misaligned(d, N))
        return QGTC_EALIGN;
    if (codes_bytes < static_cast<size_t>(N) * ldk || (xq && xq_bytes < codes_matrix_bytes(M, K, ldx)) || codes_dest_short(d, M, N))
        return QGTC_ESIZE;
    const ChainLeft l{x, xq, ldx, M, K, reinterpret_cast<const float4 *>(qa), static_cast<float>((1 << a_bits) - 1)};
    const AlinRight w{codes_t, ldk, N, reinterpret_cast<const float4 *>(qb), groups_b == N && N > 1 ? 1 : 0, col_sums, row_scale, bias, relu ? 1 : 0};
    const AlinOut o{out, outq, ldo, d.qp(), d.qmax()};
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (x) return (K & 3) == 0 && aligned16(x) ? chain_pick<1, true>(l, w, o, st) : chain_pick<0, true>(l, w, o, st);
    const bool v16 = (ldx & 15u) == 0 && aligned16(xq);
    if (outq) return v16 ? chain_pick<3, true>(l, w, o, st) : chain_pick<2, true>(l, w, o, st);
    return v16 ? chain_pick<3, false>(l, w, o, st) : chain_pick<2, false>(l, w, o, st);
}

int qgtc_tiledmm_u8_requant(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const uint8_t *Q,
                            size_t ld, size_t q_bytes, int N, const float *qparams, const float *row_scale, const float *out_qp,
                            int out_bits, uint8_t *outq, size_t ldo, size_t outq_bytes, const uint32_t *row_mask, const uint32_t *nbr_mask,
                            size_t mask_words, void *stream) {
    const TiledRowIndex ix{row_ptr, kquad};
    const TiledU8In in{tiles, n_tiles, n, Q, ld, q_bytes, N, row_mask, nbr_mask, mask_words};
    return tiled_u8_requant_entry(ix, in, qparams, row_scale, {nullptr, 0, outq, ldo, outq_bytes, out_qp, out_bits}, stream);
}

int qgtc_tiledmm_u8_t_requant(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles, int64_t n_tiles,
                              int n, const uint8_t *Q, size_t ld, size_t q_bytes, int N, const float *qparams, const float *row_scale,
                              const float *out_qp, int out_bits, uint8_t *outq, size_t ldo, size_t outq_bytes, const uint32_t *row_mask,
                              const uint32_t *nbr_mask, size_t mask_words, void *stream) {
    const TiledColIndex ix{col_ptr, col_tile, col_rb};
    const TiledU8In in{tiles, n_tiles, n, Q, ld, q_bytes, N, row_mask, nbr_mask, mask_words};
    return tiled_u8_requant_entry(ix, in, qparams, row_scale, {nullptr, 0, outq, ldo, outq_bytes, out_qp, out_bits}, stream);
}
