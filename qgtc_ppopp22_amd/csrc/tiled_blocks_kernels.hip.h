// tiled_blocks_kernels.hip.h — part of libqgtc_hip.so (included by qgtc_tiled_blocks.hip): the kernels of mini-batch sampling on the tiled
// adjacency (include/qgtc_blocks.h) - the fixed-fanout selection of an induced subgraph and the frontier of a
// sample as a node bitmap. No atomics and no clear anywhere: every output word is written once with a plain store.
//
// Selection. tiled_fanout_kernels.hip.h's scheme - one wavefront per node, count, then the k-th largest hash MSB first over registers, LDS
// or a re-walk - over walks that carry the neighbour bitmap: the row walk ANDs the four bitmap words of a tile's k-quad into the tile row
// before the decode (as tiled_nodes.hip.h does), the column walk asks for the row bit of the lane's tile row. What a walk hands out is
// exactly the node's cells in the induced subgraph, so the count is deg_m and chooses the path. A wave whose node is outside the row
// bitmap walks nothing and stores 0 / 0; it still meets the barrier. The parent's kernel is left as it is; with two null bitmaps this
// one computes its words.
//
// Frontier. The output is indexed by the neighbour, so the kernels walk the OTHER view's index and every workgroup owns whole output words:
//   k_tiled_fanout_frontier    row-axis sample; one workgroup per k-quad (4 output words) walks the k-quad's tile list, a half-wave per
//                              entry, lane r on tile row r: kept cells are ORed into 4 accumulators a lane, then across the wave with
//                              cross-lane ORs and across the 4 waves through LDS.
//   k_tiled_fanout_frontier_t  column-axis sample; one workgroup per 32-row block (1 output word) walks the block's tiles, a half-wave per
//                              tile: "my row kept a cell" is one flag a lane, a ballot gives the half-waves' words.
#pragma once

#include "tiled_fanout_kernels.hip.h"
#include "tiled_nodes.hip.h"

namespace {

// FanoutRowWalk under a neighbour bitmap (null: all)
struct FanoutRowWalkNodes {
    FanoutRowWalk w;
    const uint32_t *nbr;
    template <class F>
    __device__ __forceinline__ void operator()(int i, int lane, const TiledDrop &d, F &&f) const {
        if (w.n_tiles == 0) return;
        const int rb = i >> 5, r = i & 31, nq = step128(w.n);
        const uint64_t t0 = static_cast<uint64_t>(w.row_ptr[rb]);
        uint64_t t1 = static_cast<uint64_t>(w.row_ptr[rb + 1]);
        t1 = t1 < w.n_tiles ? t1 : w.n_tiles;
        const uint32_t R = tiled_drop_row_half(d, static_cast<uint32_t>(i));
        for (uint64_t t = t0 + lane; t < t1; t += 64) {
            const int q = w.kquad[t];
            if (static_cast<unsigned>(q) >= static_cast<unsigned>(nq)) continue;
            const uint4 a = *reinterpret_cast<const uint4 *>(w.tiles + t * 128 + r * 4);
            const uint4 b = nbr ? *reinterpret_cast<const uint4 *>(nbr + q * 4) : make_uint4(~0u, ~0u, ~0u, ~0u);   // q differs by lane
            const uint32_t word[4] = {a.x & b.x, a.y & b.y, a.z & b.z, a.w & b.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                uint32_t m = word[k];
                while (m) {
                    const int bit = __builtin_clz(m);
                    m &= ~(0x80000000u >> bit);
                    const int v = q * 128 + k * 32 + bit;
                    if (v < w.n) f(tiled_drop_mix32((R ^ tiled_drop_col_half(d, static_cast<uint32_t>(v))) + d.K));
                }
            }
        }
    }
};

// FanoutColWalk under a neighbour bitmap: the neighbour of column j in tile row r of row block rb is node rb * 32 + r
struct FanoutColWalkNodes {
    FanoutColWalk w;
    const uint32_t *nbr;
    template <class F>
    __device__ __forceinline__ void operator()(int j, int lane, const TiledDrop &d, F &&f) const {
        if (w.n_tiles == 0) return;
        const int q = j >> 7, c = j & 127, kw = c >> 5, sh = 31 - (c & 31), r = lane & 31, nrb = (w.n + 31) / 32;
        const uint64_t b0 = static_cast<uint64_t>(w.col_ptr[q]);
        uint64_t t1 = static_cast<uint64_t>(w.col_ptr[q + 1]);
        t1 = t1 < w.n_tiles ? t1 : w.n_tiles;
        const uint32_t C = tiled_drop_col_half(d, static_cast<uint32_t>(j));
        for (uint64_t e = b0 + (lane >> 5); e < t1; e += 2) {
            const uint64_t t = static_cast<uint64_t>(w.col_tile[e]);
            const int rb = w.col_rb[e];
            if (t >= w.n_tiles || static_cast<unsigned>(rb) >= static_cast<unsigned>(nrb)) continue;
            if (nbr && !tiled_nodes_bit(nbr[rb], r)) continue;   // rb < S32(n) <= S128(n) * 4
            const uint32_t word = w.tiles[t * 128 + r * 4 + kw];
            const int i = rb * 32 + r;
            if (((word >> sh) & 1u) && i < w.n) f(tiled_drop_mix32((tiled_drop_row_half(d, static_cast<uint32_t>(i)) ^ C) + d.K));
        }
    }
};

// k_tiled_fanout_thr's selection for the node of this wave: (thr, deg). `sel` is wave-uniform; a wave without a node to select for walks
// nothing. Every wave of the workgroup calls this once: it holds the workgroup's one barrier.
template <class Walk>
__device__ __forceinline__ uint32_t tiled_fanout_select(const Walk &walk, int u, bool sel, int lane, uint32_t k, const TiledDrop &d,
                                                        uint32_t *mine, uint32_t &deg) {
    uint32_t cnt = 0;
    if (sel) walk(u, lane, d, [&](uint32_t) { ++cnt; });
    uint32_t incl = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = static_cast<uint32_t>(__shfl_up(static_cast<int>(incl), o, 64));
        if (lane >= o) incl += up;
    }
    deg = static_cast<uint32_t>(__shfl(static_cast<int>(incl), 63, 64));
    const bool select = deg > k, in_lds = select && deg <= static_cast<uint32_t>(FANOUT_LDS);
    if (in_lds) {
        uint32_t at = incl - cnt;
        walk(u, lane, d, [&](uint32_t h) {
            if (at < static_cast<uint32_t>(FANOUT_LDS)) mine[at] = h;
            ++at;
        });
    }
    __syncthreads();
    uint32_t T = 0;
    if (select) {
        const bool one_each = deg <= 64u;
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
    return T;
}

template <class Walk>
__global__ __launch_bounds__(256) void k_tiled_fanout_thr_nodes(Walk walk, int n, uint32_t k, TiledDrop d,
                                                                const uint32_t *__restrict__ row_mask, uint32_t *__restrict__ thr,
                                                                int32_t *__restrict__ kept) {
    __shared__ uint32_t held[4][FANOUT_LDS];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t u64 = static_cast<int64_t>(blockIdx.x) * 4 + wave;
    const bool live = u64 < n;
    const int u = live ? static_cast<int>(u64) : 0;
    const bool sel = live && tiled_nodes_bit(tiled_nodes_word(row_mask, u >> 5), u & 31);
    uint32_t deg;
    const uint32_t T = tiled_fanout_select(walk, u, sel, lane, k, d, held[wave], deg);
    if (live && lane == 0) {
        thr[u] = T;
        if (kept) kept[u] = static_cast<int32_t>(deg < k ? deg : k);   // deg is 0 without a walk
    }
}

// the bits of word `wi` of a bitmap that stand for nodes below n
__device__ __forceinline__ uint32_t tiled_blocks_valid(int wi, int n) {
    const int64_t base = static_cast<int64_t>(wi) * 32;
    return base + 32 <= n ? 0xffffffffu : (base >= n ? 0u : 0xffffffffu << (32 - (n - base)));
}

// grid: S128(n) workgroups
__global__ __launch_bounds__(256) void k_tiled_fanout_frontier(const int64_t *__restrict__ col_ptr, const int64_t *__restrict__ col_tile,
                                                               const int32_t *__restrict__ col_rb, const uint32_t *__restrict__ tiles,
                                                               uint64_t n_tiles, int n, TiledDrop d, const uint32_t *__restrict__ thr,
                                                               const uint32_t *__restrict__ row_mask, const uint32_t *__restrict__ nbr_mask,
                                                               const uint32_t *__restrict__ include, uint32_t *__restrict__ out) {
    __shared__ uint32_t part[4][4];
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = tid & 31, hw = tid >> 5;
    const int nrb = (n + 31) / 32;
    uint32_t acc[4] = {0u, 0u, 0u, 0u};
    const uint4 nb = tiled_nodes_quad(nbr_mask, q);
    if (n_tiles != 0 && (nb.x | nb.y | nb.z | nb.w) != 0) {
        const uint64_t b0 = static_cast<uint64_t>(col_ptr[q]);
        uint64_t t1 = static_cast<uint64_t>(col_ptr[q + 1]);
        t1 = t1 < n_tiles ? t1 : n_tiles;
        for (uint64_t e = b0 + hw; e < t1; e += 8) {
            const uint64_t t = static_cast<uint64_t>(col_tile[e]);
            const int rb = col_rb[e];
            if (t >= n_tiles || static_cast<unsigned>(rb) >= static_cast<unsigned>(nrb)) continue;
            const uint32_t rw = row_mask ? row_mask[rb] : 0xffffffffu;   // the same for the half-wave: no bit, no tile load
            const int i = rb * 32 + r;
            if (!tiled_nodes_bit(rw, r) || i >= n) continue;
            const uint4 a = *reinterpret_cast<const uint4 *>(tiles + t * 128 + r * 4);
            const uint32_t w[4] = {a.x & nb.x, a.y & nb.y, a.z & nb.z, a.w & nb.w};
            const uint32_t T = thr[i], R = tiled_drop_row_half(d, static_cast<uint32_t>(i));
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                uint32_t m = w[k];
                if (T == 0) {   // every cell of the row is kept
                    acc[k] |= m;
                    continue;
                }
                while (m) {
                    const int bit = __builtin_clz(m);
                    m &= ~(0x80000000u >> bit);
                    const uint32_t v = static_cast<uint32_t>(q * 128 + k * 32 + bit);
                    if (tiled_drop_mix32((R ^ tiled_drop_col_half(d, v)) + d.K) >= T) acc[k] |= 0x80000000u >> bit;
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int o = 32; o; o >>= 1) acc[k] |= static_cast<uint32_t>(__shfl_xor(static_cast<int>(acc[k]), o, 64));
        if (lane == 0) part[wave][k] = acc[k];
    }
    __syncthreads();
    if (tid < 4) {
        const int wi = q * 4 + tid;
        uint32_t word = part[0][tid] | part[1][tid] | part[2][tid] | part[3][tid];
        if (include) word |= include[wi];
        out[wi] = word & tiled_blocks_valid(wi, n);   // a cell past n (a foreign tile) or a pad bit of include sets nothing
    }
}

// grid: S128(n) * 4 workgroups, one per output word; the words past the last row block are pad words
__global__ __launch_bounds__(256) void k_tiled_fanout_frontier_t(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ kquad,
                                                                 const uint32_t *__restrict__ tiles, uint64_t n_tiles, int n, TiledDrop d,
                                                                 const uint32_t *__restrict__ thr, const uint32_t *__restrict__ row_mask,
                                                                 const uint32_t *__restrict__ nbr_mask,
                                                                 const uint32_t *__restrict__ include, uint32_t *__restrict__ out) {
    __shared__ uint32_t part[4];
    const int rb = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = tid & 31, hw = tid >> 5;
    const int nrb = (n + 31) / 32, nq = step128(n);
    bool flag = false;
    if (n_tiles != 0 && rb < nrb) {
        const uint32_t nw = tiled_nodes_word(nbr_mask, rb);
        const int i = rb * 32 + r;
        const bool mine = tiled_nodes_bit(nw, r) && i < n;
        if (nw != 0) {
            const uint64_t t0 = static_cast<uint64_t>(row_ptr[rb]);
            uint64_t t1 = static_cast<uint64_t>(row_ptr[rb + 1]);
            t1 = t1 < n_tiles ? t1 : n_tiles;
            const uint32_t R = tiled_drop_row_half(d, static_cast<uint32_t>(i));
            for (uint64_t t = t0 + hw; t < t1; t += 8) {
                const int q = kquad[t];
                if (static_cast<unsigned>(q) >= static_cast<unsigned>(nq)) continue;
                const uint4 rm = row_mask ? *reinterpret_cast<const uint4 *>(row_mask + q * 4) : make_uint4(~0u, ~0u, ~0u, ~0u);
                if ((rm.x | rm.y | rm.z | rm.w) == 0 || !mine || flag) continue;   // no sampled column in this k-quad: no tile load
                const uint4 a = *reinterpret_cast<const uint4 *>(tiles + t * 128 + r * 4);
                const uint32_t w[4] = {a.x & rm.x, a.y & rm.y, a.z & rm.z, a.w & rm.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    uint32_t m = w[k];
                    while (m && !flag) {
                        const int bit = __builtin_clz(m);
                        m &= ~(0x80000000u >> bit);
                        const int j = q * 128 + k * 32 + bit;
                        if (j < n && tiled_drop_mix32((R ^ tiled_drop_col_half(d, static_cast<uint32_t>(j))) + d.K) >= thr[j]) flag = true;
                    }
                }
            }
        }
    }
    const uint64_t b = __ballot(flag);   // lane l of a half-wave is tile row l: bit 31 - l of the word
    if (lane == 0) part[wave] = __brev(static_cast<uint32_t>(b)) | __brev(static_cast<uint32_t>(b >> 32));
    __syncthreads();
    if (tid == 0) {
        uint32_t word = part[0] | part[1] | part[2] | part[3];
        if (include) word |= include[rb];
        out[rb] = word & tiled_blocks_valid(rb, n);
    }
}

// ---- the host side --------------------------------------------------------------------------------------------------------------------
inline int tiled_fanout_thr_nodes_args_ok(bool index_ok, const uint32_t *tiles, int64_t n_tiles, int n, int k, const uint32_t *thr,
                                          size_t thr_elems, const int32_t *kept, size_t kept_elems, const uint32_t *row_mask,
                                          const uint32_t *nbr_mask, size_t mask_words) {
    const int rc = tiled_fanout_thr_args_ok(index_ok, tiles, n_tiles, n, k, thr, thr_elems);
    if (rc == QGTC_EINVAL || rc == QGTC_EALIGN) return rc;
    if ((reinterpret_cast<uintptr_t>(kept) & 3u) != 0) return QGTC_EALIGN;
    if (rc != QGTC_OK) return rc;
    if (kept && kept_elems < static_cast<size_t>(n)) return QGTC_ESIZE;
    return tiled_nodes_args_ok(row_mask, nbr_mask, mask_words, n);
}

template <class Walk>
int tiled_fanout_thr_nodes_launch(const Walk &walk, int n, int k, uint64_t seed, const uint32_t *row_mask, uint32_t *thr, int32_t *kept,
                                  void *stream) {
    hipLaunchKernelGGL((k_tiled_fanout_thr_nodes<Walk>), dim3((n + 3) / 4), dim3(256), 0, static_cast<hipStream_t>(stream), walk, n,
                       static_cast<uint32_t>(k), tiled_drop_make(0u, seed), row_mask, thr, kept);
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

inline int tiled_fanout_frontier_args_ok(bool index_ok, const uint32_t *tiles, int64_t n_tiles, int n, const uint32_t *thr,
                                         const uint32_t *row_mask, const uint32_t *nbr_mask, const uint32_t *include, size_t mask_words,
                                         const uint32_t *out, size_t out_words) {
    if (!thr || !out || tiled_adj_malformed(index_ok, tiles, n_tiles, n)) return QGTC_EINVAL;
    if (tiled_adj_misaligned(tiles) || (reinterpret_cast<uintptr_t>(thr) & 3u) != 0 || !aligned16(out) || !aligned16(include) ||
        !aligned16(row_mask) || !aligned16(nbr_mask))
        return QGTC_EALIGN;
    const size_t need = static_cast<size_t>(step128(n)) * 4;
    if (out_words < need || ((row_mask || nbr_mask || include) && mask_words < need)) return QGTC_ESIZE;
    return QGTC_OK;
}

}  // namespace
