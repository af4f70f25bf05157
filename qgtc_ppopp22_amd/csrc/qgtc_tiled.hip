// qgtc_tiled.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): the tile-compressed adjacency of a
// whole graph (tiled_kernels.hip.h) - the two-phase packer from a raw edge list and the product requant(A_tiled . X) - and their
// launchers. The packer's sort and scans are rocPRIM's.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "qgtc.h"

#include "common.hip.h"
#include "bitmm_popcount.hip.h"   // requant (templates only: nothing is instantiated here)
#include "tiled_kernels.hip.h"

namespace {

// bytes of rocPRIM temporary storage for n_edges keys: the larger of the sort's and the scan's (the queries look at the current
// device; false when they fail)
bool tiled_temp_bytes(size_t e, size_t &bytes) {
    size_t sort_bytes = 0, scan_bytes = 0;
    if (rocprim::radix_sort_keys(nullptr, sort_bytes, static_cast<const uint64_t *>(nullptr), static_cast<uint64_t *>(nullptr), e, 0,
                                 TILED_KEY_BITS) != hipSuccess ||
        rocprim::exclusive_scan(nullptr, scan_bytes, static_cast<const uint64_t *>(nullptr), static_cast<uint64_t *>(nullptr),
                                static_cast<uint64_t>(0), e, rocprim::plus<uint64_t>()) != hipSuccess)
        return false;
    bytes = sort_bytes > scan_bytes ? sort_bytes : scan_bytes;
    return true;
}

// work buffer: [keys A | keys B | keys C] (n_edges 64-bit words each) then the temporary storage at a 256-byte boundary
size_t tiled_temp_offset_bytes(size_t e) { return (3 * e * sizeof(uint64_t) + 255) & ~static_cast<size_t>(255); }

}  // namespace

size_t qgtc_tiled_work_words(size_t n_edges) {
    size_t temp = 0;
    if (n_edges == 0 || !tiled_temp_bytes(n_edges, temp)) return 0;
    return (tiled_temp_offset_bytes(n_edges) + temp + 3) / 4;
}

int qgtc_tiled_count(const int64_t *src, const int64_t *dst, size_t n_edges, int n, int64_t *row_ptr, uint32_t *work,
                     size_t work_words, int *bad_index, void *stream) {
    if (!row_ptr || n < 1 || n > TILED_MAX_N || (n_edges && (!src || !dst || !work))) return QGTC_EINVAL;
    if (n_edges && work_words < qgtc_tiled_work_words(n_edges)) return QGTC_ESIZE;
    if (reinterpret_cast<uintptr_t>(work) & 255u) return QGTC_EALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nq = step128(n), nrb = (n + 31) / 32;
    FILL_TRY(row_ptr, 0, (nrb + 1) * sizeof(int64_t), st);
    if (bad_index) FILL_TRY(bad_index, 0, sizeof(int), st);
    if (!n_edges) return QGTC_OK;
    const uint64_t e = n_edges;
    uint64_t *A = reinterpret_cast<uint64_t *>(work), *B = A + e, *C = B + e;
    void *temp = reinterpret_cast<char *>(work) + tiled_temp_offset_bytes(e);
    size_t temp_bytes = 0;
    if (!tiled_temp_bytes(e, temp_bytes)) return QGTC_ENODEVICE;
    const int g = tiled_grid_1d(e);
    hipLaunchKernelGGL(k_tiled_keys, dim3(g), dim3(256), 0, st, src, dst, e, n, nq, A, bad_index);
    HIP_TRY(rocprim::radix_sort_keys(temp, temp_bytes, A, B, e, 0, TILED_KEY_BITS, st));
    hipLaunchKernelGGL(k_tiled_flags, dim3(g), dim3(256), 0, st, B, e, C);
    HIP_TRY(rocprim::exclusive_scan(temp, temp_bytes, C, A, static_cast<uint64_t>(0), e, rocprim::plus<uint64_t>(), st));
    FILL_TRY(C, 0xFF, e * sizeof(uint64_t), st);
    hipLaunchKernelGGL(k_tiled_compact, dim3(g), dim3(256), 0, st, B, A, e, C);
    hipLaunchKernelGGL(k_tiled_starts, dim3(g), dim3(256), 0, st, C, e, A);
    HIP_TRY(rocprim::exclusive_scan(temp, temp_bytes, A, B, static_cast<uint64_t>(0), e, rocprim::plus<uint64_t>(), st));
    hipLaunchKernelGGL(k_tiled_row_ptr, dim3(g), dim3(256), 0, st, C, A, B, e, nq, nrb, row_ptr);
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

int qgtc_tiled_fill(size_t n_edges, int n, int64_t n_tiles, int32_t *kquad, uint32_t *tiles, const uint32_t *work,
                    size_t work_words, void *stream) {
    if (n < 1 || n > TILED_MAX_N || n_tiles < 0 || (n_tiles && (!kquad || !tiles || !work)) ||
        static_cast<uint64_t>(n_tiles) > n_edges)
        return QGTC_EINVAL;
    if (n_tiles == 0) return QGTC_OK;
    if (work_words < qgtc_tiled_work_words(n_edges)) return QGTC_ESIZE;
    if (reinterpret_cast<uintptr_t>(work) & 255u) return QGTC_EALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint64_t e = n_edges;
    const uint64_t *A = reinterpret_cast<const uint64_t *>(work), *B = A + e, *C = B + e;
    FILL_TRY(tiles, 0, static_cast<size_t>(n_tiles) * 512, st);
    hipLaunchKernelGGL(k_tiled_fill, dim3(tiled_grid_1d(e)), dim3(256), 0, st, C, A, B, e, step128(n), static_cast<uint64_t>(n_tiles),
                       kquad, tiles);
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

int qgtc_tiledmm2bit(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const uint32_t *X,
                     size_t x_words, int N, int bit2, int output_bit, uint32_t *out, size_t out_words, void *stream) {
    const TiledRowIndex ix{row_ptr, kquad};
    return tiled_mm_entry<0>(ix, tiles, n_tiles, n, X, x_words, N, bit2, output_bit, out, out_words, stream);
}

int qgtc_tiledmm2int(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const uint32_t *X,
                     size_t x_words, int N, int bit2, float *out, size_t out_elems, void *stream) {
    const TiledRowIndex ix{row_ptr, kquad};
    return tiled_mm_entry<2>(ix, tiles, n_tiles, n, X, x_words, N, bit2, 1, out, out_elems, stream);
}
