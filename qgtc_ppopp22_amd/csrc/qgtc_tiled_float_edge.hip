// qgtc_tiled_float_edge.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): the float product of the
// tile-compressed adjacency with a value per stored cell, out[i] = row_scale[i] . sum_j values[slot(i, j)] . X[j] (the instantiations of
// tiled_float_kernels.hip.h whose pack ends in the edge values; include/qgtc.h, "Edge values"), and the three
// kernels of the value index: the tiles' bit counts with the in-tile row prefix, the slot of every edge of a list, and the cell of
// every slot.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "qgtc.h"

#include "common.hip.h"
#include "tiled_float_kernels.hip.h"

namespace {

// half a wave a tile: lane r holds tile row r; its popcount is scanned over the 32 lanes (exclusive), lane 31 has the tile's count
__global__ __launch_bounds__(256) void k_tiled_value_index(const uint32_t *__restrict__ tiles, uint64_t n_tiles, int64_t *__restrict__ counts,
                                                           int16_t *__restrict__ val_row) {
    const uint64_t t = static_cast<uint64_t>(blockIdx.x) * 8 + threadIdx.x / 32;
    const int r = threadIdx.x & 31;
    if (t >= n_tiles) return;   // whole half-waves leave; the shuffles below stay within 32 lanes
    const uint4 w = *reinterpret_cast<const uint4 *>(tiles + t * 128 + r * 4);
    const int own = __builtin_popcount(w.x) + __builtin_popcount(w.y) + __builtin_popcount(w.z) + __builtin_popcount(w.w);
    int incl = own;
#pragma unroll
    for (int d = 1; d < 32; d <<= 1) {
        const int up = __shfl_up(incl, d, 32);
        if (r >= d) incl += up;
    }
    val_row[t * 32 + r] = static_cast<int16_t>(incl - own);
    if (r == 31) counts[t] = incl;
}

// one thread an edge: the tile of (src >> 5, dst >> 7) by binary search in the row block's ascending k-quads, then the cell's bit
__global__ __launch_bounds__(256) void k_tiled_edge_slots(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ kquad,
                                                          const uint32_t *__restrict__ tiles, uint64_t n_tiles, int n,
                                                          const int64_t *__restrict__ val_ptr, const int16_t *__restrict__ val_row,
                                                          const int64_t *__restrict__ src, const int64_t *__restrict__ dst, uint64_t E,
                                                          int64_t *__restrict__ slot) {
    const uint64_t e = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (e >= E) return;
    const int64_t s = src[e], d = dst[e];
    int64_t res = -1;
    if (s >= 0 && s < n && d >= 0 && d < n && n_tiles) {
        const int rb = static_cast<int>(s >> 5), qd = static_cast<int>(d >> 7);
        uint64_t lo = static_cast<uint64_t>(row_ptr[rb]), hi = static_cast<uint64_t>(row_ptr[rb + 1]);
        hi = hi < n_tiles ? hi : n_tiles;
        lo = lo < hi ? lo : hi;
        while (lo < hi) {   // the first tile of the block whose k-quad is not below qd
            const uint64_t mid = lo + (hi - lo) / 2;
            if (kquad[mid] < qd) lo = mid + 1;
            else hi = mid;
        }
        uint64_t end = static_cast<uint64_t>(row_ptr[rb + 1]);
        end = end < n_tiles ? end : n_tiles;
        if (lo < end && kquad[lo] == qd) {
            const int r = static_cast<int>(s & 31), c = static_cast<int>(d & 127);
            const uint4 w = *reinterpret_cast<const uint4 *>(tiles + lo * 128 + r * 4);
            const uint32_t word = (c >> 5) == 0 ? w.x : (c >> 5) == 1 ? w.y : (c >> 5) == 2 ? w.z : w.w;
            if ((word >> (31 - (c & 31))) & 1u) res = val_ptr[lo] + val_row[lo * 32 + r] + tiled_edge_row_before(w.x, w.y, w.z, w.w, c);
        }
    }
    slot[e] = res;
}

// one workgroup a 32-row block, half a wave a tile (8 at a time): lane r walks the set bits of tile row r, MSB first, from its first slot
__global__ __launch_bounds__(256) void k_tiled_edge_endpoints(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ kquad,
                                                              const uint32_t *__restrict__ tiles, uint64_t n_tiles, int n,
                                                              const int64_t *__restrict__ val_ptr, const int16_t *__restrict__ val_row,
                                                              int32_t *__restrict__ row, int32_t *__restrict__ col, uint64_t n_values) {
    const int rb = blockIdx.x, r = threadIdx.x & 31;
    uint64_t t0 = static_cast<uint64_t>(row_ptr[rb]), t1 = static_cast<uint64_t>(row_ptr[rb + 1]);
    t1 = t1 < n_tiles ? t1 : n_tiles;
    for (uint64_t t = t0 + threadIdx.x / 32; t < t1; t += 8) {
        const uint4 w4 = *reinterpret_cast<const uint4 *>(tiles + t * 128 + r * 4);
        const uint32_t w[4] = {w4.x, w4.y, w4.z, w4.w};
        const int q = kquad[t];
        uint64_t s = static_cast<uint64_t>(val_ptr[t]) + static_cast<uint64_t>(val_row[t * 32 + r]);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            uint32_t m = w[k];
            while (m) {
                const int b = __builtin_clz(m);
                m &= ~(0x80000000u >> b);
                if (s < n_values) {
                    row[s] = rb * 32 + r;
                    col[s] = q * 128 + k * 32 + b;
                }
                ++s;
            }
        }
    }
}

// what the three index entries check of the adjacency
inline int tiled_edge_adj_ok(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n) {
    if (tiled_adj_malformed(TiledRowIndex{row_ptr, kquad}.ok(), tiles, n_tiles, n)) return QGTC_EINVAL;
    if (tiled_adj_misaligned(tiles)) return QGTC_EALIGN;
    return QGTC_OK;
}

}  // namespace

int qgtc_tiled_value_index(const uint32_t *tiles, int64_t n_tiles, int64_t *counts, int16_t *val_row, void *stream) {
    if (n_tiles < 0 || (n_tiles && (!tiles || !counts || !val_row))) return QGTC_EINVAL;
    if ((tiles && !aligned16(tiles)) || (reinterpret_cast<uintptr_t>(counts) & 7u) || (reinterpret_cast<uintptr_t>(val_row) & 1u))
        return QGTC_EALIGN;
    if (!n_tiles) return QGTC_OK;
    hipLaunchKernelGGL(k_tiled_value_index, dim3(static_cast<unsigned>((n_tiles + 7) / 8)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       tiles, static_cast<uint64_t>(n_tiles), counts, val_row);
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

int qgtc_tiled_edge_slots(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n,
                          const int64_t *val_ptr, const int16_t *val_row, const int64_t *src, const int64_t *dst, size_t n_edges,
                          int64_t *slot, void *stream) {
    int rc = tiled_edge_rc(tiled_edge_adj_ok(row_ptr, kquad, tiles, n_tiles, n), tiled_edge_index_ok(val_ptr, val_row, n_tiles, 0));
    if ((n_edges && (!src || !dst || !slot)) || (n_edges + 255) / 256 > 0x7fffffffu) rc = QGTC_EINVAL;
    else if (rc == QGTC_OK && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(slot)) & 7u))
        rc = QGTC_EALIGN;
    if (rc != QGTC_OK) return rc;
    if (!n_edges) return QGTC_OK;
    hipLaunchKernelGGL(k_tiled_edge_slots, dim3(static_cast<unsigned>((n_edges + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), row_ptr, kquad, tiles, static_cast<uint64_t>(n_tiles), n, val_ptr, val_row, src, dst,
                       static_cast<uint64_t>(n_edges), slot);
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

int qgtc_tiled_edge_endpoints(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n,
                              const int64_t *val_ptr, const int16_t *val_row, int32_t *row, int32_t *col, size_t n_values, void *stream) {
    int rc = tiled_edge_rc(tiled_edge_adj_ok(row_ptr, kquad, tiles, n_tiles, n), tiled_edge_index_ok(val_ptr, val_row, n_tiles, n_values));
    if (n_values && (!row || !col)) rc = QGTC_EINVAL;
    else if (rc == QGTC_OK && (!aligned4(row) || !aligned4(col))) rc = QGTC_EALIGN;
    if (rc != QGTC_OK) return rc;
    if (!n_tiles || !n_values) return QGTC_OK;
    hipLaunchKernelGGL(k_tiled_edge_endpoints, dim3((n + 31) / 32), dim3(256), 0, static_cast<hipStream_t>(stream), row_ptr, kquad, tiles,
                       static_cast<uint64_t>(n_tiles), n, val_ptr, val_row, row, col, static_cast<uint64_t>(n_values));
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

int qgtc_tiledmm_f32_edge(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *X,
                          size_t x_elems, int N, const float *row_scale, float *out, size_t out_elems, const int64_t *val_ptr,
                          const int16_t *val_row, const float *values, size_t n_values, void *stream) {
    const TiledRowIndex ix{row_ptr, kquad};
    const int rc = tiled_edge_rc(tiled_f32_args_ok(ix.ok(), tiles, n_tiles, n, X, x_elems, N, row_scale, out, out_elems, values),
                                 n_tiles > 0 && !values ? QGTC_EINVAL : tiled_edge_index_ok(val_ptr, val_row, n_tiles, n_values));
    if (rc != QGTC_OK) return rc;
    return tiled_mm_f32_run(ix, tiles, n_tiles, n, X, N, row_scale, out, stream, TiledEdge{val_ptr, val_row, values, static_cast<int>(n_values)});
}
