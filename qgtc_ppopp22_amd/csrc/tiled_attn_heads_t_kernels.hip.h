// tiled_attn_heads_t_kernels.hip.h — part of libqgtc_hip.so (included by the qgtc_tiled_attn_heads_t*.hip units, after
// tiled_t_kernels.hip.h, tiled_float_kernels.hip.h, tiled_max_kernels.hip.h, tiled_attn_kernels.hip.h, tiled_attn_t_kernels.hip.h and
// tiled_attn_heads_kernels.hip.h): the attention product and the score gradient for H heads on the column view of the tile-compressed
// adjacency (include/qgtc_attn_heads.h).
//
// k_tiled_att_f32_t's and k_tiled_att_grad_t's workgroups, with the transposer role of tiled_attn_t_kernels.hip.h (TiledAttStagerOf) used
// as it is. The state a row group takes from LDS and puts back each round:
//   product   the 128 x W running sums of the chunk's W = 16 * CPL columns, lane l on the ADJACENT columns l * CPL .. + CPL - 1, and in
//             the forward one den per (output row, head in the chunk): CPL is at most d, so a chunk touches at most 17 heads. Every
//             lane reads the den of its columns' heads; the lane that holds a head's first column of the chunk writes it back.
//   gradient  one float per (output row, head of the workgroup): at most 64 heads, the 64 / P of one slot.
#pragma once

namespace {

constexpr int TILED_ATTH_HC = 17;   // heads a chunk of 16 * CPL columns can touch when CPL <= d: 16 whole ones and a split one's two ends

template <int CPL, bool BWD, bool ONE, class... Drop>
__global__ __launch_bounds__(256) void k_tiled_att_heads_f32_t(const int64_t *__restrict__ col_ptr, const int64_t *__restrict__ col_tile,
                                                               const int32_t *__restrict__ col_rb, const uint32_t *__restrict__ tiles,
                                                               uint64_t n_tiles, int n, const float *__restrict__ X, int N, TiledAttH at,
                                                               float *__restrict__ m_out, float *__restrict__ inv_out,
                                                               float *__restrict__ out, Drop... drop) {
    constexpr int LPR = 16, G = 256 / LPR, TS = TILED_T_TS, HC = TILED_ATTH_HC;
    static_assert(TS == 8, "an output row reads its 8 masks of a round as two uint4");
    constexpr int W = LPR * CPL;   // output columns per workgroup
    __shared__ __attribute__((aligned(16))) uint32_t mk[128 * TS];   // [tile column][staged tile]
    __shared__ int srb[TS];
    __shared__ __attribute__((aligned(16))) float acc[128 * W];
    __shared__ float dn[BWD ? 1 : 128 * HC];
    __shared__ int lists[G][TILED_F32_CAP];
    const int q = blockIdx.x, tid = threadIdx.x;
    const int g = tid / LPR, l = tid % LPR, c0 = blockIdx.y * W + l * CPL;
    int *list = lists[g];
    int hh[CPL];
    tiled_atth_heads_of<CPL>(hh, c0, N, at.d);
    const int h0 = (blockIdx.y * W) / at.d;   // the chunk's first head
    [[maybe_unused]] bool keeps[CPL];         // this lane holds the first column the chunk has of the column's head
#pragma unroll
    for (int cc = 0; cc < CPL; ++cc) keeps[cc] = c0 + cc < N && ((c0 + cc) % at.d == 0 || (l == 0 && cc == 0));
    for (int j = g; j < 128; j += G) {
#pragma unroll
        for (int cc = 0; cc < CPL; ++cc) acc[j * W + l * CPL + cc] = 0.0f;
        if constexpr (!BWD)
            for (int k = l; k < HC; k += LPR) dn[j * HC + k] = 0.0f;
    }

    uint64_t b0 = 0, t1 = 0;   // an adjacency without tiles may come without col_ptr
    constexpr bool NODES = tiled_has_nodes<Drop...>();
    [[maybe_unused]] const TiledNodes nodes = tiled_nodes_of(drop...);
    [[maybe_unused]] uint4 rw = make_uint4(0, 0, 0, 0);   // the row bitmap's words of this k-quad
    bool walk = n_tiles != 0;
    if constexpr (NODES) {
        rw = tiled_nodes_quad(nodes.row, q);
        walk = walk && (rw.x | rw.y | rw.z | rw.w) != 0;
    }
    if (walk) {
        b0 = static_cast<uint64_t>(col_ptr[q]);
        t1 = static_cast<uint64_t>(col_ptr[q + 1]);
        t1 = t1 < n_tiles ? t1 : n_tiles;
    }
    TiledAttStagerOf<NODES> stg{col_tile, col_rb, tiles, n_tiles, t1, 0, (n + 31) / 32, tid & 31, tid >> 5, -1, -1, make_uint4(0, 0, 0, 0)};
    if constexpr (NODES) {
        stg.nbr = nodes.nbr;
        stg.rw = rw;
    }
    stg.start(b0);
    for (uint64_t base = b0; base < t1; base += TS) {
        stg.stage(base, mk, srb);
        __syncthreads();
        for (int j = g; j < 128; j += G) {
            const int self = q * 128 + j;
            if (self >= n) break;
            const uint4 ma = *reinterpret_cast<const uint4 *>(mk + j * TS), mb = *reinterpret_cast<const uint4 *>(mk + j * TS + 4);
            const uint32_t m[TS] = {ma.x, ma.y, ma.z, ma.w, mb.x, mb.y, mb.z, mb.w};
            if (!(ma.x | ma.y | ma.z | ma.w | mb.x | mb.y | mb.z | mb.w)) continue;
            float s[CPL], den[CPL];
#pragma unroll
            for (int cc = 0; cc < CPL; ++cc) {
                s[cc] = acc[j * W + l * CPL + cc];
                den[cc] = 0.0f;
                if constexpr (!BWD) den[cc] = dn[j * HC + hh[cc] - h0];
            }
            int cnt = 0;
#pragma unroll
            for (int st = 0; st < TS; ++st)
                if (m[st]) tiled_atth_decode<CPL, BWD, ONE>(m[st], srb[st] * 32, n, s, den, list, cnt, X, N, c0, at, hh, self, tiled_drop_for(self, drop)...);
            tiled_atth_add_rows<CPL, BWD, ONE>(s, den, list, cnt, X, N, c0, at, hh, self);
#pragma unroll
            for (int cc = 0; cc < CPL; ++cc) {
                acc[j * W + l * CPL + cc] = s[cc];
                if constexpr (!BWD)
                    if (keeps[cc]) dn[j * HC + hh[cc] - h0] = den[cc];
            }
        }
        __syncthreads();
    }
    __syncthreads();   // an empty list: the zeros above

    for (int j = g; j < 128; j += G) {
        const int row = q * 128 + j;
        if (row >= n) break;
#pragma unroll
        for (int cc = 0; cc < CPL; ++cc) {
            const int c = c0 + cc;
            if (c < N) {
                const float s = acc[j * W + l * CPL + cc];
                float inv = 1.0f;
                if constexpr (!BWD) {
                    const float den = dn[j * HC + hh[cc] - h0];
                    inv = den > 0.0f ? __fdiv_rn(1.0f, den) : 0.0f;
                    if (c % at.d == 0) {
                        const uint64_t sh = static_cast<uint64_t>(row) * at.H + hh[cc];
                        m_out[sh] = tiled_att_shift(at.a.own[sh], at.a.shift[sh], at.a.slope);
                        inv_out[sh] = inv;
                    }
                }
                out[static_cast<uint64_t>(row) * N + c] = BWD ? s : tiled_att_mul(s, inv);
            }
        }
    }
}

// the score gradient on the column view: tiled_atth_grad_rows with a wave per output row, the running sums of the workgroup's heads of
// every row in LDS between rounds (every lane of a head's group computes the same word; the group's first lane writes it)
template <int NS, bool WIDE, bool NBR_OWNS, class... Drop>
__global__ __launch_bounds__(256) void k_tiled_att_heads_grad_t(const int64_t *__restrict__ col_ptr, const int64_t *__restrict__ col_tile,
                                                                const int32_t *__restrict__ col_rb, const uint32_t *__restrict__ tiles,
                                                                uint64_t n_tiles, int n, const float *__restrict__ A,
                                                                const float *__restrict__ B, int N, TiledAttH at, float *__restrict__ out,
                                                                Drop... drop) {
    constexpr int G = 4, TS = TILED_T_TS, R = NS ? NS : 1, S = WIDE ? 1 : NS;
    constexpr int HB = WIDE ? 1 : 64 * NS;   // heads a workgroup can hold: NS slots of at most 64 heads
    static_assert(TS == 8, "an output row reads its 8 masks of a round as two uint4");
    static_assert(WIDE || NS != 0, "the narrow mapping keeps its slots in registers");
    __shared__ __attribute__((aligned(16))) uint32_t mk[128 * TS];   // [tile column][staged tile]
    __shared__ int srb[TS];
    __shared__ float acc[128 * HB];
    __shared__ int lists[G][TILED_F32_CAP];
    const int q = blockIdx.x, tid = threadIdx.x;
    const int g = __builtin_amdgcn_readfirstlane(tid / 64), l = tid % 64;
    int *list = lists[g];
    TiledAttHLane<R, WIDE> ln;
    ln.make(at, blockIdx.y, l);
    int at_lds[S];   // where the head of slot k keeps its sum, within a row's HB floats
#pragma unroll
    for (int k = 0; k < S; ++k) at_lds[k] = WIDE ? 0 : (l + 64 * k) >> at.lg;
    for (int i = tid; i < 128 * HB; i += 256) acc[i] = 0.0f;

    uint64_t b0 = 0, t1 = 0;   // an adjacency without tiles may come without col_ptr
    constexpr bool NODES = tiled_has_nodes<Drop...>();
    [[maybe_unused]] const TiledNodes nodes = tiled_nodes_of(drop...);
    [[maybe_unused]] uint4 rw = make_uint4(0, 0, 0, 0);   // the row bitmap's words of this k-quad
    bool walk = n_tiles != 0;
    if constexpr (NODES) {
        rw = tiled_nodes_quad(nodes.row, q);
        walk = walk && (rw.x | rw.y | rw.z | rw.w) != 0;
    }
    if (walk) {
        b0 = static_cast<uint64_t>(col_ptr[q]);
        t1 = static_cast<uint64_t>(col_ptr[q + 1]);
        t1 = t1 < n_tiles ? t1 : n_tiles;
    }
    TiledAttStagerOf<NODES> stg{col_tile, col_rb, tiles, n_tiles, t1, 0, (n + 31) / 32, tid & 31, tid >> 5, -1, -1, make_uint4(0, 0, 0, 0)};
    if constexpr (NODES) {
        stg.nbr = nodes.nbr;
        stg.rw = rw;
    }
    stg.start(b0);
    __syncthreads();
    for (uint64_t base = b0; base < t1; base += TS) {
        stg.stage(base, mk, srb);
        __syncthreads();
        for (int j = g; j < 128; j += G) {
            const int self = q * 128 + j;
            if (self >= n) break;
            const uint4 ma = *reinterpret_cast<const uint4 *>(mk + j * TS), mb = *reinterpret_cast<const uint4 *>(mk + j * TS + 4);
            const uint32_t m[TS] = {ma.x, ma.y, ma.z, ma.w, mb.x, mb.y, mb.z, mb.w};
            if (!(ma.x | ma.y | ma.z | ma.w | mb.x | mb.y | mb.z | mb.w)) continue;
            const float *__restrict__ Arow = A + static_cast<uint64_t>(self) * N;
            float own[R], s[S];
#pragma unroll
            for (int k = 0; k < R; ++k) own[k] = NS != 0 && ln.col[k] >= 0 ? Arow[ln.col[k]] : 0.0f;
#pragma unroll
            for (int k = 0; k < S; ++k) s[k] = acc[j * HB + at_lds[k]];
            int cnt = 0;
#pragma unroll
            for (int st = 0; st < TS; ++st)
                if (m[st])
                    tiled_atth_grad_decode<NS, WIDE, NBR_OWNS>(m[st], srb[st] * 32, n, s, own, ln, Arow, list, cnt, B, N, l, at, self,
                                                               tiled_drop_for(self, drop)...);
            tiled_atth_grad_rows<NS, WIDE, NBR_OWNS>(s, own, ln, Arow, list, cnt, B, N, l, at, self);
#pragma unroll
            for (int k = 0; k < S; ++k)
                if (ln.first[k]) acc[j * HB + at_lds[k]] = s[k];
        }
        __syncthreads();
    }
    __syncthreads();
    for (int j = g; j < 128; j += G) {
        const int row = q * 128 + j;
        if (row >= n) break;
#pragma unroll
        for (int k = 0; k < S; ++k)
            if (ln.first[k]) out[static_cast<uint64_t>(row) * at.H + ln.hd[k]] = acc[j * HB + at_lds[k]];
    }
}

// ---- the launchers on the column view: tiled_atth_f32_launch and tiled_atth_grad_launch ----------------------------------------------------
// the chunk is the transposed float product's (tiled_col_width_switch), narrowed until a lane's CPL columns fit in one head's d
template <bool BWD, class... Drop>
int tiled_atth_f32_launch(const TiledColIndex &ix, const uint32_t *tiles, int64_t n_tiles, int n, const float *X, int N,
                          const TiledAttH &at, float *m, float *inv, float *out, hipStream_t st, Drop... drop) {
    tiled_col_width_switch(at.d >= 4 ? N : (at.d >= 2 ? (N < 32 ? N : 32) : 16), [&](auto cpl) {
        constexpr int CPL = decltype(cpl)::value;
        const dim3 grid = tiled_col_grid(n, N, 16 * CPL);
        const uint64_t nt = static_cast<uint64_t>(n_tiles);
        if constexpr (CPL > 1) {
            if (tiled_atth_one_head(at, X, N, CPL)) {
                hipLaunchKernelGGL((k_tiled_att_heads_f32_t<CPL, BWD, true, Drop...>), grid, dim3(256), 0, st, ix.col_ptr, ix.col_tile, ix.col_rb,
                                   tiles, nt, n, X, N, at, m, inv, out, drop...);
                return;
            }
        }
        hipLaunchKernelGGL((k_tiled_att_heads_f32_t<CPL, BWD, false, Drop...>), grid, dim3(256), 0, st, ix.col_ptr, ix.col_tile, ix.col_rb,
                           tiles, nt, n, X, N, at, m, inv, out, drop...);
    });
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

template <bool NBR_OWNS, class... Drop>
int tiled_atth_grad_launch(const TiledColIndex &ix, const uint32_t *tiles, int64_t n_tiles, int n, const float *A, const float *B, int N,
                           const TiledAttH &at, const TiledAttHShape &sh, float *out, hipStream_t st, Drop... drop) {
    const dim3 block(256), grid(step128(n), sh.ny);
    tiled_atth_grad_switch(sh, [&](auto ns, auto wide) {
        hipLaunchKernelGGL((k_tiled_att_heads_grad_t<decltype(ns)::value, decltype(wide)::value, NBR_OWNS, Drop...>), grid, block, 0, st,
                           ix.col_ptr, ix.col_tile, ix.col_rb, tiles, static_cast<uint64_t>(n_tiles), n, A, B, N, at, out, drop...);
    });
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

}  // namespace
