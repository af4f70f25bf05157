// qgtc_tiled_addscore_grad_t.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): the gradient folds of the
// additive edge score over the COLUMNS of the tile-compressed adjacency, d_own[j, c] = att[c] . sum_i dL(u) . g[slot(i, j) * H + c / d]
// and P[j, c] = sum_i g[slot(i, j) * H + c / d] . L(u), u = own[j, c] + nbr[i, c] (the column-view kernel of
// tiled_addscore_grad_kernels.hip.h; include/qgtc_addscore.h). g is the row view's array: a cell's slot does not
// depend on the view.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "qgtc_addscore.h"

#include "common.hip.h"
#include "bitmm_popcount.hip.h"   // requant, for tiled_t_kernels.hip.h (templates only: nothing is instantiated here)
#include "tiled_t_kernels.hip.h"  // the in-register bit transpose
#include "tiled_float_kernels.hip.h"
#include "tiled_attn_kernels.hip.h"   // the leaky relu and the unfused multiply (templates only)
#define QGTC_TILED_ADDSCORE_T 1       // the column view's kernel of the shared header
#include "tiled_addscore_grad_kernels.hip.h"

int qgtc_tiled_addscore_grad_heads_f32_t(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                                         int64_t n_tiles, int n, const float *own, const float *nbr, size_t x_elems, int N,
                                         const float *att, size_t att_elems, float negative_slope, float *d_own, float *P,
                                         size_t out_elems, const int64_t *val_ptr, const int16_t *val_row, const float *g,
                                         size_t n_values, int heads, void *stream) {
    return tiled_addscore_grad_entry(TiledColIndex{col_ptr, col_tile, col_rb}, tiles, n_tiles, n, own, nbr, x_elems, N, att, att_elems,
                                     negative_slope, d_own, P, out_elems, val_ptr, val_row, g, n_values, heads, stream);
}
