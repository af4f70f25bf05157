// qgtc_tiled_float_nodes.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): the float product of the
// tile-compressed adjacency under node masks, out = diag(row_scale) . (A_tiled restricted to row_mask x nbr_mask) . diag(src_scale) . X
// (the instantiations of tiled_float_kernels.hip.h whose pack ends in the masks; include/qgtc.h, "Node masks"; DESIGN.md section
// 6.15e), and the kernel that turns byte flags into a node bitmap.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "qgtc.h"

#include "common.hip.h"
#include "tiled_float_kernels.hip.h"

namespace {

// one thread a word: flags 32 w .. 32 w + 31, MSB first; flags from n up do not exist and give zero bits, so pad bits and pad words are 0
__global__ __launch_bounds__(256) void k_node_bitmap(const uint8_t *__restrict__ flags, int n, uint32_t *__restrict__ words, int n_words) {
    const int w = blockIdx.x * 256 + threadIdx.x;
    if (w >= n_words) return;
    uint32_t m = 0;
    const int base = w * 32;
#pragma unroll 8
    for (int i = 0; i < 32; ++i)
        if (base + i < n && flags[base + i]) m |= 0x80000000u >> i;
    words[w] = m;
}

}  // namespace

int qgtc_node_bitmap(const uint8_t *flags, int n, uint32_t *words, size_t words_len, void *stream) {
    if (!flags || !words || n < 1 || n > TILED_MAX_N) return QGTC_EINVAL;
    if (!aligned16(words)) return QGTC_EALIGN;
    const int n_words = step128(n) * 4;
    if (words_len < static_cast<size_t>(n_words)) return QGTC_ESIZE;
    hipLaunchKernelGGL(k_node_bitmap, dim3((n_words + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), flags, n, words, n_words);
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

int qgtc_tiledmm_f32_nodes(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *X,
                           size_t x_elems, int N, const float *row_scale, const float *src_scale, float *out, size_t out_elems,
                           const uint32_t *row_mask, const uint32_t *nbr_mask, size_t mask_words, void *stream) {
    const TiledRowIndex ix{row_ptr, kquad};
    int rc = tiled_f32_args_ok(ix.ok(), tiles, n_tiles, n, X, x_elems, N, row_scale, out, out_elems, src_scale);
    if (rc == QGTC_OK) rc = tiled_nodes_args_ok(row_mask, nbr_mask, mask_words, n);
    if (rc != QGTC_OK) return rc;
    return tiled_mm_f32_masked(ix, tiles, n_tiles, n, X, N, row_scale, src_scale, out, stream, TiledNodes{row_mask, nbr_mask});
}
