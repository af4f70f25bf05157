// qgtc_tiled_float_fanout.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): the float product of the
// tile-compressed adjacency over a fixed-fanout sample, out = diag(row_scale) . (A_tiled sampled) . diag(src_scale) . X (the
// instantiations of tiled_float_kernels.hip.h whose pack ends in the fanout mask, own and nbr form; include/qgtc_fanout.h; DESIGN.md
// section 6.15l).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "qgtc_fanout.h"

#include "common.hip.h"
#include "tiled_fanout.hip.h"
#include "tiled_float_kernels.hip.h"

int qgtc_tiledmm_f32_fanout(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *X,
                            size_t x_elems, int N, const float *row_scale, const float *src_scale, float *out, size_t out_elems,
                            const uint32_t *thr, int thr_of_nbr, uint64_t seed, void *stream) {
    const TiledRowIndex ix{row_ptr, kquad};
    const int rc = tiled_fanout_args_ok(tiled_f32_args_ok(ix.ok(), tiles, n_tiles, n, X, x_elems, N, row_scale, out, out_elems, src_scale),
                                        thr, thr_of_nbr);
    if (rc != QGTC_OK) return rc;
    return tiled_fanout_run<false>(thr, thr_of_nbr, seed, n, [&](auto mask) {
        return tiled_mm_f32_masked(ix, tiles, n_tiles, n, X, N, row_scale, src_scale, out, stream, mask);
    });
}
