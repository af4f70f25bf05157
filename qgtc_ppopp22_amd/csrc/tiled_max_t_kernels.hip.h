// tiled_max_t_kernels.hip.h — part of libqgtc_hip.so (included by qgtc_tiled_max_t.hip, after tiled_t_kernels.hip.h,
// tiled_float_kernels.hip.h and tiled_max_kernels.hip.h): the extremum and its select on the column view of the tile-compressed
// adjacency, out[v] = reduce over the set cells of column v (include/qgtc.h, "Extremum tiled products").
//
// k_tiled_mm_f32_t's workgroup: one per k-quad and chunk of W = LPR * CPL output columns; the k-quad's column list is walked TS = 8
// tiles a round, each half-wave bit-transposes one tile into LDS masks, then a row group of LPR = 16 lanes takes the state of every
// output row that has a mask in the round from LDS, folds the staged tiles in order (ascending row block, each mask MSB first =
// ascending neighbour id) and puts the state back. The state is Red::WORDS arrays of 128 x W words: the running value and, for the
// extremum, the winner. Two arrays of 128 x 64 words would be 64 KB, past the static LDS of a workgroup, so the extremum runs at
// W <= 32 (the launcher cuts wider outputs into 32-column chunks) and keeps the 32 KB of the float kernel; the select has one array
// and keeps W <= 64. Node masks at the end of the pack (tiled_nodes.hip.h) act as in k_tiled_mm_f32_t: the k-quad's four row-bitmap
// words decide before the first barrier whether the list is walked, and both bitmaps are ANDed into a tile's words before the transpose.
#pragma once

namespace {

template <int LPR, int CPL, class Red, class... Drop>
__global__ __launch_bounds__(256) void k_tiled_red_f32_t(const int64_t *__restrict__ col_ptr, const int64_t *__restrict__ col_tile,
                                                         const int32_t *__restrict__ col_rb, const uint32_t *__restrict__ tiles,
                                                         uint64_t n_tiles, int n, int N, Red red, Drop... drop) {
    constexpr int G = 256 / LPR, TS = TILED_T_TS;
    static_assert(TS == 8, "an output row reads its 8 masks of a round as two uint4");
    constexpr int W = LPR * CPL;   // output columns per workgroup
    static_assert(Red::WORDS * 128 * W * 4 <= 32768, "the state of 128 rows stays within 32 KB of LDS");
    __shared__ __attribute__((aligned(16))) uint32_t mk[128 * TS];   // [tile column][staged tile]
    __shared__ int srb[TS];
    __shared__ float acc[128 * W];
    __shared__ int win[Red::WORDS == 2 ? 128 * W : 1];
    __shared__ int lists[G][TILED_F32_CAP];
    const int q = blockIdx.x, tid = threadIdx.x;
    const int g = tid / LPR;
    const int l = tid % LPR, c0 = blockIdx.y * W + l;
    const int nrb = (n + 31) / 32;
    int *list = lists[g];
    for (int j = g; j < 128; j += G)
#pragma unroll
        for (int cc = 0; cc < CPL; ++cc) {
            acc[j * W + cc * LPR + l] = 0.0f;
            if constexpr (Red::WORDS == 2) win[j * W + cc * LPR + l] = -1;
        }

    const int lane = tid & 31, s_own = tid >> 5;   // transposer role: half-wave s of the workgroup stages tile base + s
    uint64_t b0 = 0, t1 = 0;                       // an adjacency without tiles may come without col_ptr
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
    uint4 w = make_uint4(0, 0, 0, 0);
    // the loads of the transposer role run ahead of the rounds: the list entry two rounds ahead, the tile words one round ahead
    // (an entry is checked when it is used, not when it is loaded: a skipped tile or row block leaves zero masks)
    auto entry = [&](uint64_t i, uint64_t &t, int &rb) {
        t = n_tiles;
        rb = -1;
        if (i < t1) {
            t = static_cast<uint64_t>(col_tile[i]);
            rb = col_rb[i];
        }
    };
    auto words = [&](uint64_t t, int &rb) {
        if (t < n_tiles && static_cast<unsigned>(rb) < static_cast<unsigned>(nrb)) {
            uint4 r = *reinterpret_cast<const uint4 *>(tiles + t * 128 + (31 - lane) * 4);
            if constexpr (NODES) {
                const uint32_t nb = nodes.nbr ? nodes.nbr[rb] : 0xffffffffu;   // rb < S32(n) <= S128(n) * 4
                const uint32_t on = (nb >> lane) & 1u ? 0xffffffffu : 0u;
                r = make_uint4(r.x & rw.x & on, r.y & rw.y & on, r.z & rw.z & on, r.w & rw.w & on);
            }
            return r;
        }
        rb = -1;
        return make_uint4(0, 0, 0, 0);
    };
    uint64_t tn;
    int rb, rbn;
    {
        uint64_t tc;
        entry(b0 + s_own, tc, rb);
        entry(b0 + TS + s_own, tn, rbn);
        w = words(tc, rb);
    }
    for (uint64_t base = b0; base < t1; base += TS) {
        {
            uint32_t v[4] = {w.x, w.y, w.z, w.w};
            tiled_t_transpose(v, lane);
#pragma unroll
            for (int k = 0; k < 4; ++k) mk[(k * 32 + 31 - lane) * TS + s_own] = v[k];
            if (lane == 0) srb[s_own] = rb;
            rb = rbn;
            w = words(tn, rb);
            entry(base + 2 * TS + s_own, tn, rbn);
        }
        __syncthreads();
        for (int j = g; j < 128; j += G) {
            const int self = q * 128 + j;
            if (self >= n) break;
            const uint4 ma = *reinterpret_cast<const uint4 *>(mk + j * TS), mb = *reinterpret_cast<const uint4 *>(mk + j * TS + 4);
            const uint32_t m[TS] = {ma.x, ma.y, ma.z, ma.w, mb.x, mb.y, mb.z, mb.w};
            if (!(ma.x | ma.y | ma.z | ma.w | mb.x | mb.y | mb.z | mb.w)) continue;
            TiledRedState<CPL> st;
#pragma unroll
            for (int cc = 0; cc < CPL; ++cc) {
                st.s[cc] = acc[j * W + cc * LPR + l];
                st.a[cc] = Red::WORDS == 2 ? win[j * W + cc * LPR + l] : 0;
            }
            int cnt = 0;
#pragma unroll
            for (int t = 0; t < TS; ++t)
                if (m[t]) tiled_red_decode<LPR, CPL>(m[t], srb[t] * 32, n, st, self, list, cnt, red, N, c0, tiled_drop_for(self, drop)...);
            red.template rows<LPR, CPL>(st, self, list, cnt, N, c0);
#pragma unroll
            for (int cc = 0; cc < CPL; ++cc) {
                acc[j * W + cc * LPR + l] = st.s[cc];
                if constexpr (Red::WORDS == 2) win[j * W + cc * LPR + l] = st.a[cc];
            }
        }
        __syncthreads();
    }

    for (int j = g; j < 128; j += G) {
        const int row = q * 128 + j;
        if (row >= n) break;
#pragma unroll
        for (int cc = 0; cc < CPL; ++cc) {
            const int c = c0 + cc * LPR;
            if (c < N) red.store(static_cast<uint64_t>(row) * N + c, acc[j * W + cc * LPR + l], Red::WORDS == 2 ? win[j * W + cc * LPR + l] : 0);
        }
    }
}

// ---- the launcher of k_tiled_red_f32_t: tiled_red_f32_launch on the column view. The extremum keeps two words of state a column and
// stops at 32 columns a workgroup; the select keeps one and goes to 64 like the float product ----------------------------------------
template <class Red, class... Drop>
int tiled_red_f32_launch(const TiledColIndex &ix, const uint32_t *tiles, int64_t n_tiles, int n, int N, const Red &red, hipStream_t st,
                         Drop... drop) {
    static_assert(sizeof...(Drop) == 0 || Red::WORDS == 2, "a mask goes with the extremum: two words of state a column, 32 columns a workgroup");
    tiled_col_width_switch<Red::WORDS == 2 ? 32 : 64>(N, [&](auto cpl) {
        constexpr int CPL = decltype(cpl)::value;
        hipLaunchKernelGGL((k_tiled_red_f32_t<16, CPL, Red, Drop...>), tiled_col_grid(n, N, 16 * CPL), dim3(256), 0, st, ix.col_ptr,
                           ix.col_tile, ix.col_rb, tiles, static_cast<uint64_t>(n_tiles), n, N, red, drop...);
    });
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

}  // namespace
