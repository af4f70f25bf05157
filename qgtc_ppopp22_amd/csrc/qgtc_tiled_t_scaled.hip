// qgtc_tiled_t_scaled.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): the scaled transposed product
// of the tile-compressed adjacency, quantise(fl32(A_tiled^T . X) * row_scale): the entries that hand tiled_t_kernels.hip.h's launcher a
// row_scale, and with them the kernel's instantiations with that pack.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "qgtc.h"

#include "common.hip.h"
#include "bitmm_popcount.hip.h"   // requant (templates only: nothing is instantiated here)
#include "tiled_t_kernels.hip.h"

int qgtc_tiledmm2bit_t_scaled(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                              int64_t n_tiles, int n, const uint32_t *X, size_t x_words, int N, int bit2, int output_bit,
                              const float *row_scale, uint32_t *out, size_t out_words, void *stream) {
    const TiledColIndex ix{col_ptr, col_tile, col_rb};
    return tiled_mm_entry<0>(ix, tiles, n_tiles, n, X, x_words, N, bit2, output_bit, out, out_words, stream, row_scale);
}

int qgtc_tiledmm2int_t_scaled(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                              int64_t n_tiles, int n, const uint32_t *X, size_t x_words, int N, int bit2, const float *row_scale,
                              float *out, size_t out_elems, void *stream) {
    const TiledColIndex ix{col_ptr, col_tile, col_rb};
    return tiled_mm_entry<2>(ix, tiles, n_tiles, n, X, x_words, N, bit2, 1, out, out_elems, stream, row_scale);
}
