// qgtc_tiled_bit_t_nodes.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): the transposed bit products
// of the tile-compressed adjacency under node masks (include/qgtc_bitnodes.h): the instantiations of
// tiled_t_kernels.hip.h whose pack ends in the masks.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "qgtc_bitnodes.h"

#include "common.hip.h"
#include "bitmm_popcount.hip.h"   // requant (templates only: nothing is instantiated here)
#include "tiled_t_kernels.hip.h"
#include "tiled_bit_nodes.hip.h"

int qgtc_tiledmm2bit_t_nodes(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles, int64_t n_tiles,
                             int n, const uint32_t *X, size_t x_words, int N, int bit2, int output_bit, const float *row_scale,
                             uint32_t *out, size_t out_words, const uint32_t *row_mask, const uint32_t *nbr_mask, size_t mask_words,
                             void *stream) {
    const TiledColIndex ix{col_ptr, col_tile, col_rb};
    return tiled_mm_nodes_entry<0>(ix, tiles, n_tiles, n, X, x_words, N, bit2, output_bit, row_scale, out, out_words, row_mask, nbr_mask,
                                   mask_words, stream);
}

int qgtc_tiledmm2int_t_nodes(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles, int64_t n_tiles,
                             int n, const uint32_t *X, size_t x_words, int N, int bit2, const float *row_scale, float *out,
                             size_t out_elems, const uint32_t *row_mask, const uint32_t *nbr_mask, size_t mask_words, void *stream) {
    const TiledColIndex ix{col_ptr, col_tile, col_rb};
    return tiled_mm_nodes_entry<2>(ix, tiles, n_tiles, n, X, x_words, N, bit2, 1, row_scale, out, out_elems, row_mask, nbr_mask, mask_words,
                                   stream);
}
