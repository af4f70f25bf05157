// qgtc_tiled_codes.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): the byte-code route of affine
// quantisation (include/qgtc_codes.h) - the quantiser to one byte a code and the row-view entries of the
// neighbour sum of a uint8 code matrix, plain and with the dequantising epilogue, over the kernels of tiled_codes_kernels.hip.h. Every
// entry checks, makes one launch on the caller's stream and returns: no atomics, no host read, no allocation.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "qgtc_codes.h"

#include "common.hip.h"
#include "bitmm_popcount.hip.h"   // requant, for tiled_t_kernels.hip.h (templates only: nothing is instantiated here)
#include "tiled_codes_kernels.hip.h"

namespace {

template <bool VEC, bool PERCOL>
int codes_launch(const float *x, int H, int W, int nbits, const float *qparams, uint8_t *out, size_t ld, hipStream_t st) {
    const unsigned long long total = static_cast<unsigned long long>(H) * ((static_cast<unsigned long long>(W) + 3u) / 4u);
    const unsigned g = static_cast<unsigned>(tiled_grid_1d(total));
    hipLaunchKernelGGL((k_affine_codes<VEC, PERCOL>), dim3(g), dim3(256), 0, st, x, H, W, static_cast<float>((1 << nbits) - 1),
                       reinterpret_cast<const float4 *>(qparams), out, ld, g * 256u);
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

}  // namespace

int qgtc_affine_codes(const float *x, int H, int W, int nbits, const float *qparams, int groups, uint8_t *out, size_t ld, size_t out_bytes,
                      void *stream) {
    if (!x || !qparams || !out || H <= 0 || W <= 0 || nbits < 1 || nbits > 8 || (groups != 1 && groups != W)) return QGTC_EINVAL;
    if (!aligned16(qparams) || !codes_aligned4(x) || codes_matrix_misaligned(out, ld, W)) return QGTC_EALIGN;
    if (out_bytes < codes_matrix_bytes(H, W, ld)) return QGTC_ESIZE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool vec = (W & 3) == 0 && aligned16(x), percol = groups == W && W > 1;
    if (vec) return percol ? codes_launch<true, true>(x, H, W, nbits, qparams, out, ld, st) : codes_launch<true, false>(x, H, W, nbits, qparams, out, ld, st);
    return percol ? codes_launch<false, true>(x, H, W, nbits, qparams, out, ld, st) : codes_launch<false, false>(x, H, W, nbits, qparams, out, ld, st);
}

int qgtc_tiledmm_u8(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const uint8_t *Q, size_t ld,
                    size_t q_bytes, int N, int32_t *out, size_t out_elems, const uint32_t *row_mask, const uint32_t *nbr_mask,
                    size_t mask_words, void *stream) {
    const TiledRowIndex ix{row_ptr, kquad};
    return tiled_u8_entry<false>(ix, tiles, n_tiles, n, Q, ld, q_bytes, N, nullptr, nullptr, out, out_elems, row_mask, nbr_mask, mask_words,
                                 stream);
}

int qgtc_tiledmm_u8_affine(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const uint8_t *Q,
                           size_t ld, size_t q_bytes, int N, const float *qparams, const float *row_scale, float *out, size_t out_elems,
                           const uint32_t *row_mask, const uint32_t *nbr_mask, size_t mask_words, void *stream) {
    const TiledRowIndex ix{row_ptr, kquad};
    return tiled_u8_entry<true>(ix, tiles, n_tiles, n, Q, ld, q_bytes, N, qparams, row_scale, out, out_elems, row_mask, nbr_mask, mask_words,
                                stream);
}
