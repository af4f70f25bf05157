// qgtc_tiled_codes_linear.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): the C entry of
// include/qgtc_fused.h - the re-quantising walk of the static affine chain and the byte-code product behind it
// in one launch, over k_tiled_mm_u8_lin of tiled_codes_linear_kernels.hip.h. The entry checks, makes one launch on the caller's stream
// and returns: no atomics, no host read, no allocation.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "qgtc_fused.h"

#include "common.hip.h"
#include "affine_kernels.hip.h"          // aquant: the quantiser itself
#include "affine_linear_kernels.hip.h"   // the constants of the byte-code product
#include "affine_chain_kernels.hip.h"    // alin_stage, alin_step, alin_epilogue
#include "bitmm_popcount.hip.h"          // requant, for tiled_t_kernels.hip.h (templates only: nothing is instantiated here)
#include "tiled_codes_kernels.hip.h"     // the walk's decoder, adder and epilogue
#include "tiled_codes_linear_kernels.hip.h"

namespace {

template <int LPR, int NT, bool OUTQ>
int tcl_launch(const TiledRowIndex &ix, const TiledU8In &a, int K, const TclWalk &h, const AlinRight &w, const AlinOut &o, hipStream_t st) {
    hipLaunchKernelGGL((k_tiled_mm_u8_lin<LPR, NT, OUTQ>), dim3((a.n + 31) / 32), dim3(256), tcl_lds(K, NT), st, ix.row_ptr, ix.kquad,
                       a.tiles, static_cast<uint64_t>(a.n_tiles), a.n, K, h, w, o, TiledNodes{a.row_mask, a.nbr_mask});
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

// NT: the accumulators a wave needs for all of W's column tiles (half of them, the waves split them odd and even), halved until s_h and
// the 2 NT tiles of a pass fit the budget - then the tiles go in passes
template <int LPR, bool OUTQ>
int tcl_pick(const TiledRowIndex &ix, const TiledU8In &a, int K, const TclWalk &h, const AlinRight &w, const AlinOut &o, hipStream_t st) {
    const int per_wave = ((w.N + 15) / 16 + 1) / 2;
    int nt = per_wave <= 1 ? 1 : per_wave <= 2 ? 2 : per_wave <= 4 ? 4 : 8;
    while (nt > 1 && tcl_lds(K, nt) > static_cast<size_t>(TCL_LDS_BUDGET)) nt >>= 1;
    switch (nt) {
        case 1: return tcl_launch<LPR, 1, OUTQ>(ix, a, K, h, w, o, st);
        case 2: return tcl_launch<LPR, 2, OUTQ>(ix, a, K, h, w, o, st);
        case 4: return tcl_launch<LPR, 4, OUTQ>(ix, a, K, h, w, o, st);
        default:
            if constexpr (LPR < 64) return tcl_launch<LPR, 8, OUTQ>(ix, a, K, h, w, o, st);   // (K > 128: 8 never fits beside s_h)
            return QGTC_EINVAL;
    }
}

template <bool OUTQ>
int tcl_width(const TiledRowIndex &ix, const TiledU8In &a, int K, const TclWalk &h, const AlinRight &w, const AlinOut &o, hipStream_t st) {
    if (K <= 64) return tcl_pick<16, OUTQ>(ix, a, K, h, w, o, st);
    if (K <= 128) return tcl_pick<32, OUTQ>(ix, a, K, h, w, o, st);
    return tcl_pick<64, OUTQ>(ix, a, K, h, w, o, st);
}

}  // namespace

int qgtc_tiledmm_u8_linear(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const uint8_t *Q,
                           size_t ld, size_t q_bytes, int K, const float *t_qparams, const float *agg_row_scale, const float *h_qp,
                           int h_bits, const uint8_t *codes_t, size_t ldk, size_t codes_bytes, int N2, const float *qb, int groups_b,
                           const int32_t *col_sums, const float *lin_row_scale, const float *bias, int relu, float *out, size_t out_elems,
                           uint8_t *outq, size_t ldo, size_t outq_bytes, const float *out_qp, int out_bits, const uint32_t *row_mask,
                           const uint32_t *nbr_mask, size_t mask_words, void *stream) {
    const TiledRowIndex ix{row_ptr, kquad};
    const TiledU8In in{tiles, n_tiles, n, Q, ld, q_bytes, K, row_mask, nbr_mask, mask_words};
    const CodesDest d{out, out_elems, outq, ldo, outq_bytes, out_qp, out_bits};
    if (tiled_u8_invalid(ix, in) || codes_dest_invalid(d) || !t_qparams || !h_qp || !codes_t || !qb || !col_sums || K > QGTC_FUSED_K_MAX ||
        N2 < 1 || N2 > QGTC_FUSED_N_MAX || h_bits < 1 || h_bits > 8 || (groups_b != 1 && groups_b != N2))
        return QGTC_EINVAL;
    const bool w_off = !aligned16(codes_t) || ldk < static_cast<size_t>(K) || (ldk & 15u) != 0;
    if (tiled_u8_misaligned(in) || codes_dest_misaligned(d, N2) || !aligned16(t_qparams) || !aligned16(h_qp) ||
        !codes_aligned4(agg_row_scale) || w_off || !aligned16(qb) || !codes_aligned4(col_sums) || !codes_aligned4(lin_row_scale) ||
        !codes_aligned4(bias))
        return QGTC_EALIGN;
    if (tiled_u8_short(in) || codes_dest_short(d, n, N2) || codes_bytes < static_cast<size_t>(N2) * ldk) return QGTC_ESIZE;
    const TclWalk h{Q, ld, reinterpret_cast<const float4 *>(t_qparams), agg_row_scale, reinterpret_cast<const float4 *>(h_qp),
                    static_cast<float>((1 << h_bits) - 1)};
    const AlinRight w{codes_t, ldk, N2, reinterpret_cast<const float4 *>(qb), groups_b == N2 && N2 > 1 ? 1 : 0, col_sums, lin_row_scale, bias,
                      relu ? 1 : 0};
    const AlinOut o{out, outq, ldo, d.qp(), d.qmax()};
    hipStream_t st = static_cast<hipStream_t>(stream);
    return outq ? tcl_width<true>(ix, in, K, h, w, o, st) : tcl_width<false>(ix, in, K, h, w, o, st);
}
