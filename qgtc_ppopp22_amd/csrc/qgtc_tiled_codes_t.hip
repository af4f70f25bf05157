// qgtc_tiled_codes_t.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): the column-view entries of the
// neighbour sum of a uint8 code matrix on the tile-compressed adjacency, out = A_tiled^T . Q, plain and with the dequantising epilogue
// (include/qgtc_codes.h; the kernels are tiled_codes_kernels.hip.h's). The masks are relative to the view:
// row_mask names output rows (A's columns).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "qgtc_codes.h"

#include "common.hip.h"
#include "bitmm_popcount.hip.h"   // requant, for tiled_t_kernels.hip.h (templates only: nothing is instantiated here)
#include "tiled_codes_kernels.hip.h"

int qgtc_tiledmm_u8_t(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles, int64_t n_tiles, int n,
                      const uint8_t *Q, size_t ld, size_t q_bytes, int N, int32_t *out, size_t out_elems, const uint32_t *row_mask,
                      const uint32_t *nbr_mask, size_t mask_words, void *stream) {
    const TiledColIndex ix{col_ptr, col_tile, col_rb};
    return tiled_u8_entry<false>(ix, tiles, n_tiles, n, Q, ld, q_bytes, N, nullptr, nullptr, out, out_elems, row_mask, nbr_mask, mask_words,
                                 stream);
}

int qgtc_tiledmm_u8_t_affine(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles, int64_t n_tiles,
                             int n, const uint8_t *Q, size_t ld, size_t q_bytes, int N, const float *qparams, const float *row_scale,
                             float *out, size_t out_elems, const uint32_t *row_mask, const uint32_t *nbr_mask, size_t mask_words,
                             void *stream) {
    const TiledColIndex ix{col_ptr, col_tile, col_rb};
    return tiled_u8_entry<true>(ix, tiles, n_tiles, n, Q, ld, q_bytes, N, qparams, row_scale, out, out_elems, row_mask, nbr_mask, mask_words,
                                stream);
}
