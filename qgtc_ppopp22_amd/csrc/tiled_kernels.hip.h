// tiled_kernels.hip.h — part of libqgtc_hip.so (included by qgtc_tiled.hip and qgtc_tiled_scaled.hip): the tile-compressed adjacency of a
// whole graph (include/qgtc.h, "Tile-compressed adjacency"; DESIGN.md sections 4 and 6.10) - its packer, its product and, at the foot,
// the product's launcher.
//
// Format: a one-plane n x n adjacency as the OCCUPIED 512-byte tiles [32 rows][4 words] of its 32-row x 128-column grid, block-sparse
// like BSR: row_ptr[32-row block] (int64, S32(n) + 1 entries), kquad[tile] (ascending within a row block), tiles[tile][32][4].
//
// Packer: every edge becomes a 47-bit cell key (tile << 12 | row in block << 7 | column in k-quad), tile = block * S128(n) + k-quad, so
// that one radix sort orders the cells by (block, k-quad, word); a run of equal keys is one cell and its length the multiplicity, and
// the cell is set when the run is 1 or >= 3 long (the 1-bit quantiser of the summed matrix, the words qgtc_pack_edge_list gives). The
// set cells are compacted, the first cell of every tile is flagged, and one exclusive scan of those flags numbers the tiles.
#pragma once

#include "tiled_args.hip.h"
#include "tiled_nodes.hip.h"

namespace {

constexpr uint64_t TILED_INVALID = ~0ull;   // key of a skipped edge: sorts after every valid key (bit 46 is set)
constexpr unsigned TILED_KEY_BITS = 47;     // tile < 2^18 * 2^16 at n <= 2^23, shifted by 12

__device__ __forceinline__ uint64_t tiled_tile(uint64_t key) { return key >> 12; }

__global__ void k_tiled_keys(const int64_t *__restrict__ src, const int64_t *__restrict__ dst, uint64_t n_edges, int n, int nq,
                             uint64_t *__restrict__ keys, int *__restrict__ bad_index) {
    for (uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x; i < n_edges;
         i += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
        const int64_t s = src[i], d = dst[i];
        uint64_t key = TILED_INVALID;
        if (s >= 0 && s < n && d >= 0 && d < n)
            key = ((static_cast<uint64_t>(s >> 5) * nq + static_cast<uint64_t>(d >> 7)) << 12) | (static_cast<uint64_t>(s & 31) << 7) |
                  static_cast<uint64_t>(d & 127);
        else if (bad_index)
            *bad_index = 1;
        keys[i] = key;
    }
}

// sorted[i] is the first element of its run and the run's length (the cell's multiplicity) is 1 or >= 3
__device__ __forceinline__ bool tiled_cell_set(const uint64_t *__restrict__ sorted, uint64_t i, uint64_t e) {
    const uint64_t v = sorted[i];
    if (v == TILED_INVALID || (i > 0 && sorted[i - 1] == v)) return false;
    return i + 1 >= e || sorted[i + 1] != v || (i + 2 < e && sorted[i + 2] == v);
}

__global__ void k_tiled_flags(const uint64_t *__restrict__ sorted, uint64_t e, uint64_t *__restrict__ flags) {
    for (uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x; i < e; i += static_cast<uint64_t>(gridDim.x) * blockDim.x)
        flags[i] = tiled_cell_set(sorted, i, e) ? 1u : 0u;
}

// cells (pre-filled with TILED_INVALID) <- the set cells in key order
__global__ void k_tiled_compact(const uint64_t *__restrict__ sorted, const uint64_t *__restrict__ pos, uint64_t e,
                                uint64_t *__restrict__ cells) {
    for (uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x; i < e; i += static_cast<uint64_t>(gridDim.x) * blockDim.x)
        if (tiled_cell_set(sorted, i, e)) cells[pos[i]] = sorted[i];
}

// starts[j] = cells[j] is the first set cell of its tile
__global__ void k_tiled_starts(const uint64_t *__restrict__ cells, uint64_t e, uint64_t *__restrict__ starts) {
    for (uint64_t j = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x; j < e; j += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
        const uint64_t v = cells[j];
        starts[j] = (v != TILED_INVALID && (j == 0 || tiled_tile(cells[j - 1]) != tiled_tile(v))) ? 1u : 0u;
    }
}

// row_ptr (cleared by the launcher): the first tile of block rb writes row_ptr[rb] and the entries of the empty blocks before it;
// the last set cell writes T into row_ptr[rb + 1 .. nrb]. tidx = exclusive scan of starts.
__global__ void k_tiled_row_ptr(const uint64_t *__restrict__ cells, const uint64_t *__restrict__ starts, const uint64_t *__restrict__ tidx,
                                uint64_t e, int nq, int nrb, int64_t *__restrict__ row_ptr) {
    for (uint64_t j = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x; j < e; j += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
        const uint64_t v = cells[j];
        if (v == TILED_INVALID) continue;
        const int rb = static_cast<int>(tiled_tile(v) / nq);
        if (starts[j]) {
            const int lo = j > 0 ? static_cast<int>(tiled_tile(cells[j - 1]) / nq) + 1 : 0;
            for (int r = lo; r <= rb; ++r) row_ptr[r] = static_cast<int64_t>(tidx[j]);
        }
        if (j + 1 == e || cells[j + 1] == TILED_INVALID) {
            const int64_t total = static_cast<int64_t>(tidx[j] + starts[j]);
            for (int r = rb + 1; r <= nrb; ++r) row_ptr[r] = total;
        }
    }
}

// kquad and the tile words (cleared by the launcher); a tile's set cells share words, hence the OR
__global__ void k_tiled_fill(const uint64_t *__restrict__ cells, const uint64_t *__restrict__ starts, const uint64_t *__restrict__ tidx,
                             uint64_t e, int nq, uint64_t n_tiles, int32_t *__restrict__ kquad, uint32_t *__restrict__ tiles) {
    for (uint64_t j = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x; j < e; j += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
        const uint64_t v = cells[j];
        if (v == TILED_INVALID) continue;
        const uint64_t t = tidx[j] + starts[j] - 1;
        if (t >= n_tiles) continue;
        if (starts[j]) kquad[t] = static_cast<int32_t>(tiled_tile(v) % nq);
        const uint32_t r = static_cast<uint32_t>(v >> 7) & 31u, c = static_cast<uint32_t>(v) & 127u;
        atomicOr(tiles + t * 128 + r * 4 + (c >> 5), 1u << (31 - (c & 31)));
    }
}

// ---- product: requant(A_tiled . X) -------------------------------------------------------------------------------------------------
// One workgroup (256 threads) per 32-row block and 128-column chunk of the output. A thread owns one column c and R rows of the block
// (R = 2 .. 16: narrow outputs split the block's rows over more threads) and keeps their sums in int32 registers: every row is exact
// (deg * (2^w - 1) < 2^31 for n <= 2^23, w <= 8). Per occupied tile it loads the w 16-byte k-quads of column c (cols layout: one
// line per column) and, for each of its rows with a set bit in the tile, ANDs and popcounts the row's 4 words with them. From R = 8
// up a wave's rows are the same for all its lanes, so the tile rows arrive by scalar loads and empty rows are skipped by a scalar
// branch. MODE 0: the requantised sums are ORed bit by bit into an LDS staging of the block's output words and stored as whole
// 16-byte granules (rows past n, columns past N: zeros); MODE 2: float32 [n, N].
//
// SCALED (include/qgtc.h, "Scaled tiled products and degrees"): the epilogue loads row_scale[row] for the
// thread's R rows (row < n only) and forms y = float(sum) * row_scale[row], one IEEE single multiply; MODE 2 stores y, MODE 0 runs
// the value quantiser quant1 on y in place of requant. `Scale` is empty - the unscaled kernel, with the arguments and the code it
// always had - or one `const float *`, row_scale, behind `out`.
//
// NODES (include/qgtc_bitnodes.h): the pack ends in a TiledNodes, the two node bitmaps (either may be null: all
// nodes). The block's rows are the one word row_mask[rb]: zero, and the workgroup reads no index, no tile and no X and runs the epilogue on
// zero sums. Per tile the four words nbr_mask[4q .. 4q + 3] are one uniform 16-byte read (a scalar load): all zero, and the tile is skipped
// before X's planes are loaded; otherwise they are ANDed into every tile row ahead of the non-zero test, and a row outside row_mask counts
// as an empty tile row. Without a TiledNodes every `if constexpr (NODES)` is discarded and the kernels are the ones that existed.
__device__ __forceinline__ const float *tiled_scale_ptr() { return nullptr; }
__device__ __forceinline__ const float *tiled_scale_ptr(const float *p) { return p; }
__device__ __forceinline__ const float *tiled_scale_ptr(const TiledNodes &) { return nullptr; }
__device__ __forceinline__ const float *tiled_scale_ptr(const float *p, const TiledNodes &) { return p; }

template <int R, int MODE, typename... Scale>
__global__ __launch_bounds__(256) void k_tiled_mm(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ kquad,
                                                  const uint32_t *__restrict__ tiles, uint64_t n_tiles, int n,
                                                  const uint32_t *__restrict__ X, uint64_t x_words, int N, int bit2, int ob,
                                                  float maxv, float maxm1, void *__restrict__ out, Scale... scale) {
    constexpr bool NODES = tiled_has_nodes<Scale...>();
    constexpr bool SCALED = sizeof...(Scale) > (NODES ? 1 : 0);
    [[maybe_unused]] const float *__restrict__ row_scale = tiled_scale_ptr(scale...);
    [[maybe_unused]] const TiledNodes nodes = tiled_nodes_of(scale...);
    constexpr int RS = 32 / R, CW = 256 / RS;   // row groups per block, columns per workgroup
    const int rb = blockIdx.x, chunk = blockIdx.y, tid = threadIdx.x;
    const int rs = CW >= 64 ? __builtin_amdgcn_readfirstlane(tid / CW) : tid / CW;
    const int c = chunk * 128 + tid % CW;
    const bool cv = c < N;
    const int nq = step128(n);
    const uint64_t line = static_cast<uint64_t>(nq) * 4, plane = static_cast<uint64_t>(pad128(N)) * line;
    int acc[R];
#pragma unroll
    for (int i = 0; i < R; ++i) acc[i] = 0;

    // with masks: the row bitmap's word of this block, and this thread's R rows of it from bit 31 down
    [[maybe_unused]] uint32_t rword = 0xffffffffu, rlive = 0xffffffffu;
    if constexpr (NODES) {
        rword = tiled_nodes_word(nodes.row, rb);
        rlive = rword << (rs * R);
    }
    const bool live = tiled_nodes_and<NODES>(true, rword != 0);   // a dead block reads no row_ptr: its tile range is empty
    uint64_t t1 = live ? static_cast<uint64_t>(row_ptr[rb + 1]) : 0;
    t1 = t1 < n_tiles ? t1 : n_tiles;
    for (uint64_t t = live ? static_cast<uint64_t>(row_ptr[rb]) : 0; t < t1; ++t) {
        const int q = kquad[t];
        if (static_cast<unsigned>(q) >= static_cast<unsigned>(nq)) continue;
        [[maybe_unused]] uint4 nb;
        if constexpr (NODES) {
            nb = tiled_nodes_quad(nodes.nbr, q);
            if (!(nb.x | nb.y | nb.z | nb.w)) continue;   // no neighbour of this k-quad takes part: X's planes stay unread
        }
        uint4 x[8];
#pragma unroll
        for (int p = 0; p < 8; ++p)
            x[p] = (cv && p < bit2) ? ldg4(X, x_words, p * plane + c * line + static_cast<uint64_t>(q) * 4) : make_uint4(0, 0, 0, 0);
        const uint4 *a = reinterpret_cast<const uint4 *>(tiles + t * 128) + rs * R;
#pragma unroll
        for (int i = 0; i < R; ++i) {
            uint4 ai = a[i];
            if constexpr (NODES) ai = make_uint4(ai.x & nb.x, ai.y & nb.y, ai.z & nb.z, ai.w & nb.w);
            if (tiled_nodes_and<NODES>((ai.x | ai.y | ai.z | ai.w) != 0, tiled_nodes_bit(rlive, i))) {
                int s = 0;
#pragma unroll
                for (int p = 0; p < 8; ++p)
                    if (p < bit2)
                        s += (__builtin_popcount(ai.x & x[p].x) + __builtin_popcount(ai.y & x[p].y) + __builtin_popcount(ai.z & x[p].z) +
                              __builtin_popcount(ai.w & x[p].w)) << p;
                acc[i] += s;
            }
        }
    }

    if constexpr (MODE == 2) {
        float *o = static_cast<float *>(out);
        if (cv) {
#pragma unroll
            for (int i = 0; i < R; ++i) {
                const int row = rb * 32 + rs * R + i;
                if (row < n) {
                    if constexpr (SCALED) o[static_cast<uint64_t>(row) * N + c] = static_cast<float>(acc[i]) * row_scale[row];
                    else o[static_cast<uint64_t>(row) * N + c] = static_cast<float>(acc[i]);
                }
            }
        }
    } else {
        __shared__ uint32_t st[32 * 32 * 4];   // [plane][row of the block][word of the chunk]
        for (int k = tid; k < ob * 128; k += 256) st[k] = 0;
        __syncthreads();
        if (cv) {
            const uint32_t keep = ob >= 32 ? ~0u : ((1u << ob) - 1u);
            const uint32_t bit = 1u << (31 - (c & 31));
            const int word = (c & 127) >> 5;
#pragma unroll
            for (int i = 0; i < R; ++i) {
                const int row = rs * R + i;
                if (rb * 32 + row >= n) continue;
                uint32_t m;
                if constexpr (SCALED) m = quant1(static_cast<float>(acc[i]) * row_scale[rb * 32 + row], maxv, maxm1) & keep;
                else m = static_cast<uint32_t>(requant(acc[i], maxv, maxm1)) & keep;
                while (m) {
                    const int b = __builtin_ctz(m);
                    m &= m - 1;
                    atomicOr(&st[(b * 32 + row) * 4 + word], bit);
                }
            }
        }
        __syncthreads();
        const int rows_out = pad8(n);
        const uint64_t wpr = static_cast<uint64_t>(step128(N)) * 4;
        uint32_t *o = static_cast<uint32_t *>(out);
        for (int k = tid; k < ob * 32; k += 256) {
            const int b = k >> 5, row = rb * 32 + (k & 31);
            if (row < rows_out)
                *reinterpret_cast<uint4 *>(o + (static_cast<uint64_t>(b) * rows_out + row) * wpr + chunk * 4) =
                    *reinterpret_cast<const uint4 *>(&st[k * 4]);
        }
    }
}

// ---- the launcher of k_tiled_mm ----------------------------------------------------------------------------------------------------------
// rows a thread owns (R) by N: the narrowest layout whose columns cover min(N, 128); launch(R) gets it as an integral constant
template <class F>
void tiled_mm_rows_switch(int N, F &&launch) {
    switch (N <= 16 ? 2 : (N <= 32 ? 4 : (N <= 64 ? 8 : 16))) {
        case 2: launch(tiled_int<2>{}); break;
        case 4: launch(tiled_int<4>{}); break;
        case 8: launch(tiled_int<8>{}); break;
        default: launch(tiled_int<16>{}); break;
    }
}

// It ends in the kernel's own trailing pack and forwards it: empty is the plain kernel, (row_scale) the scaled one, and either
// with a TiledNodes behind it the masked one (DESIGN.md sections 6.15f, 6.15n).
template <int MODE, class... Scale>
int tiled_mm_launch(const TiledRowIndex &ix, const uint32_t *tiles, int64_t n_tiles, int n, const uint32_t *X, size_t x_words, int N,
                    int bit2, int ob, void *out, hipStream_t st, Scale... scale) {
    const TiledClamp clamp(ob);
    tiled_mm_rows_switch(N, [&](auto r) {
        constexpr int R = decltype(r)::value;
        hipLaunchKernelGGL((k_tiled_mm<R, MODE, Scale...>), dim3((n + 31) / 32, R == 16 ? step128(N) : 1), dim3(256), 0, st, ix.row_ptr,
                           ix.kquad, tiles, static_cast<uint64_t>(n_tiles), n, X, static_cast<uint64_t>(x_words), N, bit2, ob, clamp.maxv,
                           clamp.maxm1, out, scale...);
    });
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

}  // namespace
