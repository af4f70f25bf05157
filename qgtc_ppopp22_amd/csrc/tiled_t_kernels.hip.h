// tiled_t_kernels.hip.h — part of libqgtc_hip.so (included by qgtc_tiled_t.hip and qgtc_tiled_t_scaled.hip, and for the bit transpose by
// qgtc_tiled_scaled.hip and the column-view float, extremum and attention units): the transposed product of the tile-compressed
// adjacency, requant(A_tiled^T . X), from the same tiles (include/qgtc.h, "Transposed tiled adjacency") - the
// column index that lists the tiles by k-quad, the product kernel and, at the foot, its launcher.
//
// Column index: one radix sort of the keys (kquad << tile_bits | tile id) orders the tiles by (k-quad, tile id); a tile id already
// orders the tiles of one k-quad by row block. k_tiled_col_index then writes col_tile, col_rb (a binary search of row_ptr) and col_ptr
// (the first entry of every k-quad writes its start and those of the empty k-quads before it; the last entry writes the end).
#pragma once

#include "tiled_args.hip.h"
#include "tiled_nodes.hip.h"

namespace {

__global__ void k_tiled_col_keys(const int32_t *__restrict__ kquad, uint64_t n_tiles, int nq, unsigned tile_bits,
                                 uint64_t *__restrict__ keys) {
    for (uint64_t t = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x; t < n_tiles;
         t += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
        const int q = kquad[t];
        // a k-quad outside 0 .. nq-1 sorts into group nq, past col_ptr[nq]: listed, never read by the product
        const uint64_t g = static_cast<unsigned>(q) < static_cast<unsigned>(nq) ? static_cast<uint64_t>(q) : static_cast<uint64_t>(nq);
        keys[t] = (g << tile_bits) | t;
    }
}

__global__ void k_tiled_col_index(const uint64_t *__restrict__ sorted, uint64_t n_tiles, unsigned tile_bits, const int64_t *__restrict__ row_ptr,
                                  int nrb, int nq, int64_t *__restrict__ col_ptr, int64_t *__restrict__ col_tile,
                                  int32_t *__restrict__ col_rb) {
    const uint64_t tmask = (1ull << tile_bits) - 1;
    for (uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x; i < n_tiles;
         i += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
        const uint64_t v = sorted[i], t = v & tmask;
        const int q = static_cast<int>(v >> tile_bits);
        // row block of tile t: the last rb with row_ptr[rb] <= t
        int lo = 0, hi = nrb;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (static_cast<uint64_t>(row_ptr[mid]) <= t) lo = mid;
            else hi = mid;
        }
        col_tile[i] = static_cast<int64_t>(t);
        col_rb[i] = lo;
        if (q >= nq) continue;
        const int qp = i > 0 ? static_cast<int>(sorted[i - 1] >> tile_bits) : -1;
        if (qp != q)
            for (int r = qp + 1; r <= q; ++r) col_ptr[r] = static_cast<int64_t>(i);
        const int qn = i + 1 < n_tiles ? static_cast<int>(sorted[i + 1] >> tile_bits) : nq;
        if (qn != q)
            for (int r = q + 1; r <= (qn < nq ? qn : nq); ++r) col_ptr[r] = static_cast<int64_t>(i + 1);
    }
}

// ---- product: requant(A_tiled^T . X) -----------------------------------------------------------------------------------------------
// One workgroup (256 threads) per k-quad q (output rows 128 q .. 128 q + 127) and 128-column chunk of the output. A thread owns one
// column c and R of the 128 rows (R = 8 .. 64: narrow outputs split the rows over more threads) and keeps their sums in int32
// registers. The k-quad's tiles are taken TS = 8 per round:
//   transpose  each half-wave loads one tile, lane l its row 31 - l (16 bytes, so the half-wave reads the 512-byte tile in one go),
//              and runs the 5-stage butterfly of a 32 x 32 bit transpose on each of the 4 words (cross-lane swaps at distance
//              16, 8, 4, 2, 1). Lane l then holds, for each word k, the tile column 32 k + 31 - l as a mask over the tile's 32 rows in
//              the cols-layout bit order (row i at bit 31 - i). The masks go to LDS, [tile][128 columns].
//   multiply   for every staged tile (row block rb) a thread loads one word per plane of X's column c, line word rb (source rows
//              32 rb .. 32 rb + 31), and for each of its rows with a non-zero mask adds sum_p popcount(mask & x_p) << p. From
//              R = 32 up a wave's rows are the same for all its lanes: the mask reads are LDS broadcasts and the skip is uniform.
// MODE 0: the requantised sums are ORed bit by bit into an LDS staging of the chunk's output words, 8 planes at a time, and stored as
// whole 16-byte granules (rows past n, columns past N: zeros); MODE 2: float32 [n, N].
constexpr int TILED_T_TS = 8;

__device__ __forceinline__ uint32_t tiled_t_stage(uint32_t v, uint32_t partner, int lane, int j, uint32_t m) {
    return (lane & j) ? (((partner >> j) & m) | (v & ~m)) : ((v & m) | ((partner & m) << j));
}

// the 5 butterfly stages on 4 words at once: stage j swaps bit j of the lane (row) index with bit j of the bit (column) index
__device__ __forceinline__ void tiled_t_transpose(uint32_t (&v)[4], int lane) {
    constexpr int J[5] = {16, 8, 4, 2, 1};
    constexpr uint32_t M[5] = {0x0000FFFFu, 0x00FF00FFu, 0x0F0F0F0Fu, 0x33333333u, 0x55555555u};
#pragma unroll
    for (int st = 0; st < 5; ++st)
#pragma unroll
        for (int k = 0; k < 4; ++k)
            v[k] = tiled_t_stage(v[k], static_cast<uint32_t>(__shfl_xor(static_cast<int>(v[k]), J[st])), lane, J[st], M[st]);
}

// SCALED: as in k_tiled_mm - y = float(sum) * row_scale[row] in the epilogue (row < n only), stored (MODE 2) or quantised by quant1
// in place of requant (MODE 0). `Scale` is empty (the unscaled kernel, arguments and code as they always were) or one `const float *`.
//
// NODES (include/qgtc_bitnodes.h): the pack ends in a TiledNodes. The k-quad's output rows are the four words
// row_mask[4q .. 4q + 3], one uniform 16-byte read: all zero, and the workgroup reads no col_ptr, no tile and no X. A masked-out output
// row's column mask is cleared as it is staged, so the multiply's non-zero test (uniform from R = 32 up) skips it as it skips an empty
// column. A staged tile's neighbours are A's rows 32 rb .., the one word nbr_mask[rb], in the bit order of the column masks and of X's line
// word: zero, and the tile is skipped before X's words are loaded; otherwise it is ANDed into X's bit2 words once per tile.
__device__ __forceinline__ const float *tiled_t_scale_ptr() { return nullptr; }
__device__ __forceinline__ const float *tiled_t_scale_ptr(const float *p) { return p; }
__device__ __forceinline__ const float *tiled_t_scale_ptr(const TiledNodes &) { return nullptr; }
__device__ __forceinline__ const float *tiled_t_scale_ptr(const float *p, const TiledNodes &) { return p; }

template <int R, int MODE, typename... Scale>
__global__ __launch_bounds__(256) void k_tiled_mm_t(const int64_t *__restrict__ col_ptr, const int64_t *__restrict__ col_tile,
                                                    const int32_t *__restrict__ col_rb, const uint32_t *__restrict__ tiles,
                                                    uint64_t n_tiles, int n, const uint32_t *__restrict__ X, uint64_t x_words, int N,
                                                    int bit2, int ob, float maxv, float maxm1, void *__restrict__ out, Scale... scale) {
    constexpr bool NODES = tiled_has_nodes<Scale...>();
    constexpr bool SCALED = sizeof...(Scale) > (NODES ? 1 : 0);
    [[maybe_unused]] const float *__restrict__ row_scale = tiled_t_scale_ptr(scale...);
    [[maybe_unused]] const TiledNodes nodes = tiled_nodes_of(scale...);
    constexpr int RS = 128 / R, CW = 256 / RS;   // row groups per k-quad, columns per workgroup
    constexpr int TS = TILED_T_TS;
    const int q = blockIdx.x, chunk = blockIdx.y, tid = threadIdx.x;
    const int rs = CW >= 64 ? __builtin_amdgcn_readfirstlane(tid / CW) : tid / CW;
    const int c = chunk * 128 + tid % CW;
    const bool cv = c < N;
    const int nq = step128(n), nrb = (n + 31) / 32;
    const uint64_t line = static_cast<uint64_t>(nq) * 4, plane = static_cast<uint64_t>(pad128(N)) * line;
    const uint64_t xcol = static_cast<uint64_t>(c) * line;
    __shared__ uint32_t mk[TS * 128];   // [staged tile][tile column]: the column's mask over the tile's 32 rows
    __shared__ int srb[TS];
    int acc[R];
#pragma unroll
    for (int i = 0; i < R; ++i) acc[i] = 0;

    // transposer role: half-wave s of the workgroup stages tile base + s
    const int lane = tid & 31, s_own = tid >> 5;
    // with masks: the row bitmap's four words of this k-quad's 128 output rows
    [[maybe_unused]] uint4 rq = make_uint4(~0u, ~0u, ~0u, ~0u);
    if constexpr (NODES) rq = tiled_nodes_quad(nodes.row, q);
    const bool live = tiled_nodes_and<NODES>(true, (rq.x | rq.y | rq.z | rq.w) != 0);   // a dead k-quad reads no col_ptr: its list is empty
    uint64_t t1 = live ? static_cast<uint64_t>(col_ptr[q + 1]) : 0;
    t1 = t1 < n_tiles ? t1 : n_tiles;
    for (uint64_t base = live ? static_cast<uint64_t>(col_ptr[q]) : 0; base < t1; base += TS) {
        {
            const uint64_t i = base + s_own;
            uint4 w = make_uint4(0, 0, 0, 0);
            int rb = -1;
            if (i < t1) {
                const uint64_t t = static_cast<uint64_t>(col_tile[i]);
                rb = col_rb[i];
                if (t < n_tiles) w = *reinterpret_cast<const uint4 *>(tiles + t * 128 + (31 - lane) * 4);
                else rb = -1;
            }
            uint32_t v[4] = {w.x, w.y, w.z, w.w};
            tiled_t_transpose(v, lane);
            if constexpr (NODES) {   // v[k] is output row 32 k + 31 - lane of the k-quad: bit `lane` of its word
                const uint32_t rw[4] = {rq.x, rq.y, rq.z, rq.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = ((rw[k] >> lane) & 1u) ? v[k] : 0u;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) mk[s_own * 128 + k * 32 + 31 - lane] = v[k];
            if (lane == 0) srb[s_own] = rb;
        }
        __syncthreads();
        const int ns = t1 - base < static_cast<uint64_t>(TS) ? static_cast<int>(t1 - base) : TS;
        for (int s = 0; s < ns; ++s) {
            const int rb = srb[s];
            if (static_cast<unsigned>(rb) >= static_cast<unsigned>(nrb)) continue;
            [[maybe_unused]] uint32_t nbw = 0xffffffffu;
            if constexpr (NODES) {
                nbw = tiled_nodes_word(nodes.nbr, rb);
                if (!nbw) continue;   // none of the tile's 32 neighbours takes part: X's words stay unread
            }
            uint32_t x[8];
#pragma unroll
            for (int p = 0; p < 8; ++p) x[p] = (cv && p < bit2) ? ldw(X, x_words, p * plane + xcol + static_cast<uint64_t>(rb)) : 0u;
            if constexpr (NODES) {
#pragma unroll
                for (int p = 0; p < 8; ++p) x[p] &= nbw;
            }
            const uint4 *mrow = reinterpret_cast<const uint4 *>(mk + s * 128 + rs * R);
#pragma unroll
            for (int i4 = 0; i4 < R / 4; ++i4) {
                const uint4 m4 = mrow[i4];
                const uint32_t mm[4] = {m4.x, m4.y, m4.z, m4.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (mm[k]) {
                        int sum = 0;
#pragma unroll
                        for (int p = 0; p < 8; ++p)
                            if (p < bit2) sum += __builtin_popcount(mm[k] & x[p]) << p;
                        acc[i4 * 4 + k] += sum;
                    }
                }
            }
        }
        __syncthreads();
    }

    if constexpr (MODE == 2) {
        float *o = static_cast<float *>(out);
        if (cv) {
#pragma unroll
            for (int i = 0; i < R; ++i) {
                const int row = q * 128 + rs * R + i;
                if (row < n) {
                    if constexpr (SCALED) o[static_cast<uint64_t>(row) * N + c] = static_cast<float>(acc[i]) * row_scale[row];
                    else o[static_cast<uint64_t>(row) * N + c] = static_cast<float>(acc[i]);
                }
            }
        }
    } else {
        __shared__ uint32_t st[8 * 128 * 4];   // [plane of the group][row of the k-quad][word of the chunk]
        const uint32_t keep = ob >= 32 ? ~0u : ((1u << ob) - 1u);
#pragma unroll
        for (int i = 0; i < R; ++i) {
            if constexpr (SCALED) {
                const int row = q * 128 + rs * R + i;
                acc[i] = row < n ? static_cast<int>(quant1(static_cast<float>(acc[i]) * row_scale[row], maxv, maxm1) & keep) : 0;
            } else {
                acc[i] = static_cast<int>(static_cast<uint32_t>(requant(acc[i], maxv, maxm1)) & keep);
            }
        }
        const uint32_t bit = 1u << (31 - (c & 31));
        const int word = (c & 127) >> 5;
        const int rows_out = pad8(n);
        const uint64_t wpr = static_cast<uint64_t>(step128(N)) * 4;
        uint32_t *o = static_cast<uint32_t *>(out);
        for (int g0 = 0; g0 < ob; g0 += 8) {
            const int np = ob - g0 < 8 ? ob - g0 : 8;
            for (int k = tid; k < np * 512; k += 256) st[k] = 0;
            __syncthreads();
            if (cv) {
#pragma unroll
                for (int i = 0; i < R; ++i) {
                    const int row = rs * R + i;
                    if (q * 128 + row >= n) continue;
                    uint32_t m = (static_cast<uint32_t>(acc[i]) >> g0) & 0xFFu;
                    while (m) {
                        const int b = __builtin_ctz(m);
                        m &= m - 1;
                        atomicOr(&st[(b * 128 + row) * 4 + word], bit);
                    }
                }
            }
            __syncthreads();
            for (int k = tid; k < np * 128; k += 256) {
                const int b = g0 + (k >> 7), row = q * 128 + (k & 127);
                if (row < rows_out)
                    *reinterpret_cast<uint4 *>(o + (static_cast<uint64_t>(b) * rows_out + row) * wpr + chunk * 4) =
                        *reinterpret_cast<const uint4 *>(&st[k * 4]);
            }
            __syncthreads();
        }
    }
}

// ---- the launcher of k_tiled_mm_t --------------------------------------------------------------------------------------------------------
// rows of the k-quad a thread owns (R) by N: the narrowest layout whose columns cover min(N, 128); launch(R) gets it as an integral
// constant
template <class F>
void tiled_mm_t_rows_switch(int N, F &&launch) {
    switch (N <= 16 ? 8 : (N <= 32 ? 16 : (N <= 64 ? 32 : 64))) {
        case 8: launch(tiled_int<8>{}); break;
        case 16: launch(tiled_int<16>{}); break;
        case 32: launch(tiled_int<32>{}); break;
        default: launch(tiled_int<64>{}); break;
    }
}

// the column view's overload of tiled_kernels.hip.h's launcher: the pack is empty or (row_scale), and either with a TiledNodes behind it
template <int MODE, class... Scale>
int tiled_mm_launch(const TiledColIndex &ix, const uint32_t *tiles, int64_t n_tiles, int n, const uint32_t *X, size_t x_words, int N,
                    int bit2, int ob, void *out, hipStream_t st, Scale... scale) {
    const TiledClamp clamp(ob);
    tiled_mm_t_rows_switch(N, [&](auto r) {
        constexpr int R = decltype(r)::value;
        hipLaunchKernelGGL((k_tiled_mm_t<R, MODE, Scale...>), dim3(step128(n), R == 64 ? step128(N) : 1), dim3(256), 0, st, ix.col_ptr,
                           ix.col_tile, ix.col_rb, tiles, static_cast<uint64_t>(n_tiles), n, X, static_cast<uint64_t>(x_words), N, bit2, ob,
                           clamp.maxv, clamp.maxm1, out, scale...);
    });
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

}  // namespace
