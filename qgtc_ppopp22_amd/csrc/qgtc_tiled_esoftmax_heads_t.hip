// qgtc_tiled_esoftmax_heads_t.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): the softmax of per-edge
// logits of H heads over each COLUMN's cells of the tile-compressed adjacency and its gradient (the column-view kernels of
// tiled_heads_esoftmax_kernels.hip.h; include/qgtc_heads.h). The vectors are the row view's: a cell's slot
// does not depend on the view. A lane owns a column and up to four heads of it; no atomics, every (slot, head) is written once.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "qgtc_heads.h"

#include "common.hip.h"
#include "bitmm_popcount.hip.h"   // requant, for tiled_t_kernels.hip.h (templates only: nothing is instantiated here)
#include "tiled_t_kernels.hip.h"  // the in-register bit transpose
#include "tiled_float_kernels.hip.h"
#include "tiled_max_kernels.hip.h"   // tiled_static_for, for tiled_attn_kernels.hip.h (templates only: nothing is instantiated here)
#include "tiled_attn_kernels.hip.h"  // EXP and the unfused subtract and multiply
#define QGTC_TILED_ESOFTMAX_T 1      // the column view's kernels of the shared headers
#include "tiled_esoftmax_kernels.hip.h"
#include "tiled_heads_esoftmax_kernels.hip.h"

int qgtc_tiled_edge_softmax_heads_f32_t(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                                        int64_t n_tiles, int n, const int64_t *val_ptr, const int16_t *val_row, const float *logits,
                                        float *alpha, size_t n_values, float *m, float *inv, int heads, void *stream) {
    const TiledColIndex ix{col_ptr, col_tile, col_rb};
    const float *const vec[] = {logits, alpha};
    const int rc = tiled_esm_heads_args_ok(ix.ok(), tiles, n_tiles, n, val_ptr, val_row, n_values, vec, m, inv, heads);
    if (rc != QGTC_OK) return rc;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (!n_tiles || !n_values) return tiled_esm_heads_no_cells(n, heads, m, inv, st);
    tiled_esm_heads_switch(heads, [&](auto hc, int gy) {
        hipLaunchKernelGGL((k_tiled_esoftmax_heads_t<decltype(hc)::value>), dim3(step128(n), gy), dim3(128), 0, st, col_ptr, col_tile, col_rb,
                           tiles, static_cast<uint64_t>(n_tiles), n, val_ptr, val_row, logits, alpha, static_cast<int>(n_values), m, inv,
                           heads);
    });
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

int qgtc_tiled_edge_softmax_grad_heads_f32_t(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb,
                                             const uint32_t *tiles, int64_t n_tiles, int n, const int64_t *val_ptr,
                                             const int16_t *val_row, const float *alpha, const float *g, float *out, size_t n_values,
                                             int heads, void *stream) {
    const TiledColIndex ix{col_ptr, col_tile, col_rb};
    const float *const vec[] = {alpha, g, out};
    const int rc = tiled_esm_heads_args_ok(ix.ok(), tiles, n_tiles, n, val_ptr, val_row, n_values, vec, nullptr, nullptr, heads);
    if (rc != QGTC_OK) return rc;
    if (!n_tiles || !n_values) return QGTC_OK;
    tiled_esm_heads_switch(heads, [&](auto hc, int gy) {
        hipLaunchKernelGGL((k_tiled_esoftmax_grad_heads_t<decltype(hc)::value>), dim3(step128(n), gy), dim3(128), 0,
                           static_cast<hipStream_t>(stream), col_ptr, col_tile, col_rb, tiles, static_cast<uint64_t>(n_tiles), n, val_ptr,
                           val_row, alpha, g, out, static_cast<int>(n_values), heads);
    });
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}
