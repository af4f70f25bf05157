// qgtc_tiled_t.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): the transposed product of the
// tile-compressed adjacency (tiled_t_kernels.hip.h) - the column index, built with one rocPRIM radix sort, and the product
// requant(A_tiled^T . X) - and their launchers.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "qgtc.h"

#include "common.hip.h"
#include "bitmm_popcount.hip.h"   // requant (templates only: nothing is instantiated here)
#include "tiled_t_kernels.hip.h"

namespace {

constexpr int64_t TILED_T_MAX_TILES = int64_t{1} << 40;   // tile ids fit 40 bits, k-quads 17: a sort key fits 57

unsigned bit_width(uint64_t v) {
    unsigned b = 0;
    while (v) ++b, v >>= 1;
    return b;
}

// work buffer: [keys A | keys B] (n_tiles 64-bit words each) then the sort's temporary storage at a 256-byte boundary. The storage
// is queried for all 64 key bits, the most any call sorts.
size_t colindex_temp_offset_bytes(size_t t) { return (2 * t * sizeof(uint64_t) + 255) & ~static_cast<size_t>(255); }

bool colindex_temp_bytes(size_t t, size_t &bytes) {
    return rocprim::radix_sort_keys(nullptr, bytes, static_cast<const uint64_t *>(nullptr), static_cast<uint64_t *>(nullptr), t, 0,
                                    64) == hipSuccess;
}

}  // namespace

size_t qgtc_tiled_colindex_work_words(int64_t n_tiles) {
    size_t temp = 0;
    if (n_tiles <= 0 || n_tiles > TILED_T_MAX_TILES || !colindex_temp_bytes(static_cast<size_t>(n_tiles), temp)) return 0;
    return (colindex_temp_offset_bytes(static_cast<size_t>(n_tiles)) + temp + 3) / 4;
}

int qgtc_tiled_colindex(const int64_t *row_ptr, const int32_t *kquad, int64_t n_tiles, int n, int64_t *col_ptr, int64_t *col_tile,
                        int32_t *col_rb, uint32_t *work, size_t work_words, void *stream) {
    if (!col_ptr || n < 1 || n > TILED_MAX_N || n_tiles < 0 || n_tiles > TILED_T_MAX_TILES ||
        (n_tiles && (!row_ptr || !kquad || !col_tile || !col_rb || !work)))
        return QGTC_EINVAL;
    if (n_tiles) {
        const size_t need = qgtc_tiled_colindex_work_words(n_tiles);
        if (!need) return QGTC_ENODEVICE;
        if (work_words < need) return QGTC_ESIZE;
    }
    if (reinterpret_cast<uintptr_t>(work) & 255u) return QGTC_EALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nq = step128(n), nrb = (n + 31) / 32;
    FILL_TRY(col_ptr, 0, (static_cast<size_t>(nq) + 1) * sizeof(int64_t), st);
    if (!n_tiles) return QGTC_OK;
    const uint64_t t = static_cast<uint64_t>(n_tiles);
    const unsigned tile_bits = bit_width(t - 1) ? bit_width(t - 1) : 1, end_bit = tile_bits + bit_width(static_cast<uint64_t>(nq));
    uint64_t *A = reinterpret_cast<uint64_t *>(work), *B = A + t;
    void *temp = reinterpret_cast<char *>(work) + colindex_temp_offset_bytes(t);
    size_t temp_bytes = 0;
    if (!colindex_temp_bytes(t, temp_bytes)) return QGTC_ENODEVICE;
    const int g = tiled_grid_1d(t);
    hipLaunchKernelGGL(k_tiled_col_keys, dim3(g), dim3(256), 0, st, kquad, t, nq, tile_bits, A);
    HIP_TRY(rocprim::radix_sort_keys(temp, temp_bytes, A, B, t, 0, end_bit, st));
    hipLaunchKernelGGL(k_tiled_col_index, dim3(g), dim3(256), 0, st, B, t, tile_bits, row_ptr, nrb, nq, col_ptr, col_tile, col_rb);
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

int qgtc_tiledmm2bit_t(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles, int64_t n_tiles,
                       int n, const uint32_t *X, size_t x_words, int N, int bit2, int output_bit, uint32_t *out, size_t out_words,
                       void *stream) {
    const TiledColIndex ix{col_ptr, col_tile, col_rb};
    return tiled_mm_entry<0>(ix, tiles, n_tiles, n, X, x_words, N, bit2, output_bit, out, out_words, stream);
}

int qgtc_tiledmm2int_t(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles, int64_t n_tiles,
                       int n, const uint32_t *X, size_t x_words, int N, int bit2, float *out, size_t out_elems, void *stream) {
    const TiledColIndex ix{col_ptr, col_tile, col_rb};
    return tiled_mm_entry<2>(ix, tiles, n_tiles, n, X, x_words, N, bit2, 1, out, out_elems, stream);
}
