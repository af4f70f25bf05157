// qgtc_reorder.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): node reordering for the
// tile-compressed adjacency (reorder_kernels.hip.h) and its launcher. The sorts are rocPRIM's.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "qgtc.h"

#include "common.hip.h"
#include "tiled_args.hip.h"   // TILED_MAX_N and the 1-D grid rule
#include "reorder_kernels.hip.h"

namespace {

size_t align256(size_t b) { return (b + 255) & ~static_cast<size_t>(255); }

// Work buffer (byte offsets, each region 256-byte aligned). K = max(2 n_edges, n) 64-bit keys in `a` and `b`: the sort of the entries,
// the sort of the nodes by class, the hash tables of the hub lists during the sweeps (2 * 2 n_edges 32-bit words) and the final sort.
struct ReorderLayout {
    size_t a, b, nbr, off, order, label, prop, size, seg, changed, temp, temp_bytes, total;
};

bool reorder_layout(int n, size_t n_edges, ReorderLayout &L) {
    const size_t m = 2 * n_edges, k = m > static_cast<size_t>(n) ? m : static_cast<size_t>(n);
    size_t sort_bytes = 0, node_bytes = 0;
    if (rocprim::radix_sort_keys(nullptr, sort_bytes, static_cast<const uint64_t *>(nullptr), static_cast<uint64_t *>(nullptr), k, 0,
                                 REORDER_KEY_BITS) != hipSuccess ||
        rocprim::radix_sort_keys(nullptr, node_bytes, static_cast<const uint64_t *>(nullptr), static_cast<uint64_t *>(nullptr),
                                 static_cast<size_t>(n), 0, REORDER_CLASS_BITS) != hipSuccess)
        return false;
    size_t p = 0;
    L.a = p, p = align256(p + k * 8);
    L.b = p, p = align256(p + k * 8);
    L.nbr = p, p = align256(p + m * 4);
    L.off = p, p = align256(p + (static_cast<size_t>(n) + 1) * 8);
    L.order = p, p = align256(p + static_cast<size_t>(n) * 4);
    L.label = p, p = align256(p + static_cast<size_t>(n) * 4);
    L.prop = p, p = align256(p + static_cast<size_t>(n) * 4);
    L.size = p, p = align256(p + static_cast<size_t>(n) * 8);   // two int32 [n]: sweep t counts into (t & 1)
    L.seg = p, p = align256(p + (REORDER_CLASSES + 1) * 4);
    L.changed = p, p = align256(p + REORDER_MAX_SWEEPS * 4);
    L.temp = p;
    L.temp_bytes = sort_bytes > node_bytes ? sort_bytes : node_bytes;
    L.total = p + L.temp_bytes;
    return true;
}

}  // namespace

size_t qgtc_reorder_work_words(int n, size_t n_edges) {
    ReorderLayout L;
    if (n < 1 || n > REORDER_MAX_N || !reorder_layout(n, n_edges, L)) return 0;
    return (L.total + 3) / 4;
}

int qgtc_reorder_nodes(const int64_t *src, const int64_t *dst, size_t n_edges, int n, int sweeps, int cap, int64_t *perm,
                       int64_t *rank, uint32_t *work, size_t work_words, int *bad_index, void *stream) {
    if (!perm || n < 1 || n > REORDER_MAX_N || sweeps < 0 || sweeps > REORDER_MAX_SWEEPS || cap < 1 ||
        (n_edges && (!src || !dst || !work)))
        return QGTC_EINVAL;
    ReorderLayout L;
    if (n_edges) {
        if (!reorder_layout(n, n_edges, L)) return QGTC_ENODEVICE;
        if (work_words < (L.total + 3) / 4) return QGTC_ESIZE;
        if (reinterpret_cast<uintptr_t>(work) & 255u) return QGTC_EALIGN;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (bad_index) FILL_TRY(bad_index, 0, sizeof(int), st);
    if (!n_edges || !sweeps) {   // no neighbour entries or no sweep: every label stays the node's own id
        if (n_edges && bad_index)
            hipLaunchKernelGGL(k_reorder_check, dim3(tiled_grid_1d(n_edges)), dim3(256), 0, st, src, dst, static_cast<uint64_t>(n_edges), n,
                               bad_index);
        hipLaunchKernelGGL(k_reorder_identity, dim3(tiled_grid_1d(n)), dim3(256), 0, st, n, perm, rank);
        HIP_TRY(hipGetLastError());
        return QGTC_OK;
    }

    char *w = reinterpret_cast<char *>(work);
    uint64_t *A = reinterpret_cast<uint64_t *>(w + L.a), *B = reinterpret_cast<uint64_t *>(w + L.b);
    uint32_t *nbr = reinterpret_cast<uint32_t *>(w + L.nbr), *order = reinterpret_cast<uint32_t *>(w + L.order);
    uint64_t *off = reinterpret_cast<uint64_t *>(w + L.off);
    uint32_t *label = reinterpret_cast<uint32_t *>(w + L.label), *prop = reinterpret_cast<uint32_t *>(w + L.prop);
    int *size = reinterpret_cast<int *>(w + L.size);
    uint32_t *seg = reinterpret_cast<uint32_t *>(w + L.seg), *changed = reinterpret_cast<uint32_t *>(w + L.changed);
    void *temp = w + L.temp;
    size_t temp_bytes = L.temp_bytes;
    const uint64_t e = n_edges, m = 2 * e;

    FILL_TRY(size, 0, static_cast<size_t>(n) * 8, st);
    FILL_TRY(changed, 0, REORDER_MAX_SWEEPS * 4, st);
    // symmetrised neighbour lists
    hipLaunchKernelGGL(k_reorder_entry_keys, dim3(tiled_grid_1d(e)), dim3(256), 0, st, src, dst, e, n, A, bad_index);
    HIP_TRY(rocprim::radix_sort_keys(temp, temp_bytes, A, B, m, 0, REORDER_KEY_BITS, st));
    hipLaunchKernelGGL(k_reorder_offsets, dim3(tiled_grid_1d(m + 1)), dim3(256), 0, st, B, m, n, off, nbr);
    // the nodes by (degree class, parity, id)
    hipLaunchKernelGGL(k_reorder_class_keys, dim3(tiled_grid_1d(n)), dim3(256), 0, st, off, n, A);
    HIP_TRY(rocprim::radix_sort_keys(temp, temp_bytes, A, B, static_cast<size_t>(n), 0, REORDER_CLASS_BITS, st));
    hipLaunchKernelGGL(k_reorder_segments, dim3(tiled_grid_1d(static_cast<uint64_t>(n) + 1)), dim3(256), 0, st, B, n, order, seg);
    hipLaunchKernelGGL(k_reorder_init, dim3(tiled_grid_1d(n)), dim3(256), 0, st, n, label);
    // the sweeps: queued without a read-back; the launches after an early stop return at once
    uint32_t *hkey = reinterpret_cast<uint32_t *>(A), *hcount = reinterpret_cast<uint32_t *>(B);
    const int g = tiled_grid_1d(static_cast<uint64_t>(n) * 4);
    for (int t = 0; t < sweeps; ++t) {
        int *cur = size + (t & 1) * static_cast<size_t>(n), *next = size + ((t + 1) & 1) * static_cast<size_t>(n);
        hipLaunchKernelGGL(k_reorder_sweep, dim3(g), dim3(256), 0, st, t, n, off, nbr, order, seg, label, prop, cur, changed, hkey,
                           hcount);
        hipLaunchKernelGGL(k_reorder_accept, dim3(tiled_grid_1d(n)), dim3(256), 0, st, t, n, cap, label, prop, cur, next, changed);
    }
    // perm = the nodes by (label, id), rank its inverse
    hipLaunchKernelGGL(k_reorder_rank_keys, dim3(tiled_grid_1d(n)), dim3(256), 0, st, label, n, A);
    HIP_TRY(rocprim::radix_sort_keys(temp, temp_bytes, A, B, static_cast<size_t>(n), 0, REORDER_KEY_BITS, st));
    hipLaunchKernelGGL(k_reorder_perm, dim3(tiled_grid_1d(n)), dim3(256), 0, st, B, n, perm, rank);
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}
