// tiled_fanout_kernels.hip.h — part of libqgtc_hip.so (included by qgtc_tiled_fanout.hip): the selection kernels of fixed-fanout
// sampling (include/qgtc_fanout.h): thr[u] = 0 when node u has at most k cells, otherwise the k-th largest of
// the cells' hashes H(i, j, seed) - exact for any degree, one launch, no atomics, plain stores, every thr[0 .. n) written.
//
// One WAVEFRONT owns one node of the axis (4 nodes a workgroup), so the result cannot depend on the launch geometry. The two axes differ
// only in how a node's cells are walked (FanoutRowWalk, FanoutColWalk: each lane is handed some of the node's cells, one hash at a time);
// the selection is written once:
//   1. every lane counts the cells it is handed; an inclusive wave scan gives the lane's offset and the node's degree;
//   2. deg <= k: thr = 0 - on real graphs most nodes end here, after one walk;
//   3. deg <= FANOUT_LDS: the walk is repeated once and the hashes land in the wave's slice of LDS at the lanes' offsets; the answer
//      is built MSB first in 32 steps, each counting the held hashes >= candidate (the largest T with count(H >= T) >= k is the k-th
//      largest; the hashes of one node are distinct, so count(H >= T) is then exactly k). With at most 64 hashes every lane keeps one
//      in a register and a step is a compare and a ballot;
//   4. otherwise (a hub) each of the 32 steps walks the node's tiles again: nothing is buffered, so no degree overflows anything.
// All waves of a workgroup meet at the one barrier between filling LDS and reading it, whatever path they take.
#pragma once

#include "tiled_args.hip.h"
#include "tiled_drop.hip.h"

namespace {

constexpr int FANOUT_LDS = 1024;   // hashes a wave holds in LDS (4 KiB; 16 KiB a workgroup)

// the cells of row i, in A's coordinates: lane l takes the row's tiles t0 + l, t0 + l + 64, ... (16 bytes of each) and decodes them
struct FanoutRowWalk {
    const int64_t *row_ptr;
    const int32_t *kquad;
    const uint32_t *tiles;
    uint64_t n_tiles;
    int n;
    template <class F>
    __device__ __forceinline__ void operator()(int i, int lane, const TiledDrop &d, F &&f) const {
        if (n_tiles == 0) return;   // an adjacency without tiles may come without row_ptr
        const int rb = i >> 5, r = i & 31, nq = step128(n);
        const uint64_t t0 = static_cast<uint64_t>(row_ptr[rb]);
        uint64_t t1 = static_cast<uint64_t>(row_ptr[rb + 1]);
        t1 = t1 < n_tiles ? t1 : n_tiles;
        const uint32_t R = tiled_drop_row_half(d, static_cast<uint32_t>(i));
        for (uint64_t t = t0 + lane; t < t1; t += 64) {
            const int q = kquad[t];
            if (static_cast<unsigned>(q) >= static_cast<unsigned>(nq)) continue;
            const uint4 a = *reinterpret_cast<const uint4 *>(tiles + t * 128 + r * 4);
            const uint32_t w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                uint32_t m = w[k];
                while (m) {
                    const int b = __builtin_clz(m);
                    m &= ~(0x80000000u >> b);
                    const int v = q * 128 + k * 32 + b;
                    if (v < n) f(tiled_drop_mix32((R ^ tiled_drop_col_half(d, static_cast<uint32_t>(v))) + d.K));
                }
            }
        }
    }
};

// the cells of column j: the two half-waves take alternate entries of the k-quad's tile list, lane r of a half its row r of the tile -
// one word, of which one bit is this column's
struct FanoutColWalk {
    const int64_t *col_ptr, *col_tile;
    const int32_t *col_rb;
    const uint32_t *tiles;
    uint64_t n_tiles;
    int n;
    template <class F>
    __device__ __forceinline__ void operator()(int j, int lane, const TiledDrop &d, F &&f) const {
        if (n_tiles == 0) return;
        const int q = j >> 7, c = j & 127, kw = c >> 5, sh = 31 - (c & 31), r = lane & 31, nrb = (n + 31) / 32;
        const uint64_t b0 = static_cast<uint64_t>(col_ptr[q]);
        uint64_t t1 = static_cast<uint64_t>(col_ptr[q + 1]);
        t1 = t1 < n_tiles ? t1 : n_tiles;
        const uint32_t C = tiled_drop_col_half(d, static_cast<uint32_t>(j));
        for (uint64_t e = b0 + (lane >> 5); e < t1; e += 2) {
            const uint64_t t = static_cast<uint64_t>(col_tile[e]);
            const int rb = col_rb[e];
            if (t >= n_tiles || static_cast<unsigned>(rb) >= static_cast<unsigned>(nrb)) continue;
            const uint32_t word = tiles[t * 128 + r * 4 + kw];
            const int i = rb * 32 + r;
            if (((word >> sh) & 1u) && i < n) f(tiled_drop_mix32((tiled_drop_row_half(d, static_cast<uint32_t>(i)) ^ C) + d.K));
        }
    }
};

__device__ __forceinline__ uint32_t fanout_wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), o, 64));
    return v;
}

template <class Walk>
__global__ __launch_bounds__(256) void k_tiled_fanout_thr(Walk walk, int n, uint32_t k, TiledDrop d, uint32_t *__restrict__ thr) {
    __shared__ uint32_t held[4][FANOUT_LDS];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t u64 = static_cast<int64_t>(blockIdx.x) * 4 + wave;
    const bool live = u64 < n;          // wave-uniform; a wave past the end walks nothing but still meets the barrier
    const int u = live ? static_cast<int>(u64) : 0;
    uint32_t *mine = held[wave];

    uint32_t cnt = 0;
    if (live) walk(u, lane, d, [&](uint32_t) { ++cnt; });
    uint32_t incl = cnt;   // inclusive scan over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = static_cast<uint32_t>(__shfl_up(static_cast<int>(incl), o, 64));
        if (lane >= o) incl += up;
    }
    const uint32_t deg = static_cast<uint32_t>(__shfl(static_cast<int>(incl), 63, 64));
    const bool select = deg > k, in_lds = select && deg <= static_cast<uint32_t>(FANOUT_LDS);
    if (in_lds) {
        uint32_t at = incl - cnt;   // < deg <= FANOUT_LDS, and the second walk hands out what the first did (the guard costs a compare)
        walk(u, lane, d, [&](uint32_t h) {
            if (at < static_cast<uint32_t>(FANOUT_LDS)) mine[at] = h;
            ++at;
        });
    }
    __syncthreads();
    uint32_t T = 0;
    if (select) {
        const bool one_each = deg <= 64u;   // at most one held hash a lane: a step is one compare and a ballot
        const bool has = one_each && static_cast<uint32_t>(lane) < deg;
        const uint32_t hv = has ? mine[lane] : 0u;
        for (int bit = 31; bit >= 0; --bit) {
            const uint32_t cand = T | (1u << bit);
            uint32_t total;
            if (one_each) {
                total = static_cast<uint32_t>(__popcll(__ballot(has && hv >= cand)));
            } else {
                uint32_t c = 0;
                if (in_lds) {
                    for (uint32_t x = lane; x < deg; x += 64) c += mine[x] >= cand ? 1u : 0u;
                } else {
                    walk(u, lane, d, [&](uint32_t h) { c += h >= cand ? 1u : 0u; });
                }
                total = fanout_wave_sum(c);
            }
            if (total >= k) T = cand;
        }
    }
    if (live && lane == 0) thr[u] = T;
}

inline int tiled_fanout_thr_args_ok(bool index_ok, const uint32_t *tiles, int64_t n_tiles, int n, int k, const uint32_t *thr,
                                    size_t thr_elems) {
    if (!thr || k < 1 || tiled_adj_malformed(index_ok, tiles, n_tiles, n)) return QGTC_EINVAL;
    if (tiled_adj_misaligned(tiles) || (reinterpret_cast<uintptr_t>(thr) & 3u) != 0) return QGTC_EALIGN;
    if (thr_elems < static_cast<size_t>(n)) return QGTC_ESIZE;
    return QGTC_OK;
}

template <class Walk>
int tiled_fanout_thr_launch(const Walk &walk, int n, int k, uint64_t seed, uint32_t *thr, void *stream) {
    hipLaunchKernelGGL((k_tiled_fanout_thr<Walk>), dim3((n + 3) / 4), dim3(256), 0, static_cast<hipStream_t>(stream), walk, n,
                       static_cast<uint32_t>(k), tiled_drop_make(0u, seed), thr);
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

}  // namespace
