// qgtc_tiled_codes_edge.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): the row-view entry of the
// edge-weighted neighbour sum on byte codes (include/qgtc_codes_edge.h), over the kernels of
// tiled_codes_edge_kernels.hip.h. The entry checks, makes one launch on the caller's stream and returns: no atomics, no host read, no
// allocation.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "qgtc_codes_edge.h"

#include "common.hip.h"
#include "bitmm_popcount.hip.h"   // requant, for tiled_t_kernels.hip.h (templates only: nothing is instantiated here)
#include "tiled_codes_edge_kernels.hip.h"

int qgtc_tiledmm_u8_edge(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const uint8_t *Q, size_t ld,
                         size_t q_bytes, int N, const float *qparams, const float *row_scale, const int64_t *val_ptr, const int16_t *val_row,
                         const float *values, size_t n_values, int heads, float *out, size_t out_elems, uint8_t *outq, size_t ldo,
                         size_t outq_bytes, const float *out_qp, int out_bits, const uint32_t *row_mask, const uint32_t *nbr_mask,
                         size_t mask_words, void *stream) {
    const TiledRowIndex ix{row_ptr, kquad};
    const TiledU8In in{tiles, n_tiles, n, Q, ld, q_bytes, N, row_mask, nbr_mask, mask_words};
    return tiled_u8_edge_entry(ix, in, qparams, row_scale, val_ptr, val_row, values, n_values, heads,
                               {out, out_elems, outq, ldo, outq_bytes, out_qp, out_bits}, stream);
}
