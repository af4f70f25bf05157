// qgtc_tiled_addscore_grad.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): the gradient folds of the
// additive edge score over the ROWS of the tile-compressed adjacency, d_own[i, c] = att[c] . sum_j dL(u) . g[slot(i, j) * H + c / d] and
// P[i, c] = sum_j g[slot(i, j) * H + c / d] . L(u), u = own[i, c] + nbr[j, c] (the row-view kernel of tiled_addscore_grad_kernels.hip.h;
// include/qgtc_addscore.h).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "qgtc_addscore.h"

#include "common.hip.h"
#include "tiled_float_kernels.hip.h"
#include "tiled_attn_kernels.hip.h"   // the leaky relu and the unfused multiply (templates only: nothing is instantiated here)
#include "tiled_addscore_grad_kernels.hip.h"

int qgtc_tiled_addscore_grad_heads_f32(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n,
                                       const float *own, const float *nbr, size_t x_elems, int N, const float *att, size_t att_elems,
                                       float negative_slope, float *d_own, float *P, size_t out_elems, const int64_t *val_ptr,
                                       const int16_t *val_row, const float *g, size_t n_values, int heads, void *stream) {
    return tiled_addscore_grad_entry(TiledRowIndex{row_ptr, kquad}, tiles, n_tiles, n, own, nbr, x_elems, N, att, att_elems, negative_slope,
                                     d_own, P, out_elems, val_ptr, val_row, g, n_values, heads, stream);
}
