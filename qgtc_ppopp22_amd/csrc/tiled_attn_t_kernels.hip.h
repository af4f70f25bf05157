// tiled_attn_t_kernels.hip.h — part of libqgtc_hip.so (included by qgtc_tiled_attn_t.hip, after tiled_t_kernels.hip.h,
// tiled_float_kernels.hip.h, tiled_max_kernels.hip.h and tiled_attn_kernels.hip.h): the attention product and the score gradient on the
// column view of the tile-compressed adjacency (include/qgtc.h, "Attention tiled products").
//
// k_tiled_mm_f32_t's workgroup: one per k-quad (128 output rows); the k-quad's column list is walked TS = 8 tiles a round, each
// half-wave bit-transposes one tile into LDS masks, then a row group takes the state of every output row that has a mask in the round
// from LDS, folds the staged tiles in order (ascending row block, each mask MSB first = ascending neighbour id) and puts it back.
//   product   a row group is 16 lanes on a chunk of W = 16 * CPL output columns; the state is the 128 x W running sums and, in the
//             forward, one den per row beside them (every lane of the group holds the same den; lane 0 keeps it);
//   gradient  a row group is a whole wave, lane j on the columns j + 64 cc, and the state is one float per output row.
// Node masks at the end of the pack (tiled_nodes.hip.h) act as in k_tiled_mm_f32_t: the k-quad's four row-bitmap words decide from
// blockIdx alone whether the list is walked, and the transposer role ANDs both bitmaps into a tile's words before the transpose.
#pragma once

namespace {

// the transposer role both kernels share: the loads run ahead of the rounds - the list entry two rounds, the tile words one round
// (an entry is checked when it is used, not when it is loaded: a skipped tile or row block leaves zero masks)
template <bool NODES>
struct TiledAttStagerOf {
    const int64_t *__restrict__ col_tile;
    const int32_t *__restrict__ col_rb;
    const uint32_t *__restrict__ tiles;
    uint64_t n_tiles, t1, tn;
    int nrb, lane, s_own, rb, rbn;
    uint4 w;
    const uint32_t *__restrict__ nbr = nullptr;   // NODES: the neighbour bitmap (or null) and the row bitmap's words of the k-quad
    uint4 rw = make_uint4(0, 0, 0, 0);

    __device__ __forceinline__ void entry(uint64_t i, uint64_t &t, int &r) const {
        t = n_tiles;
        r = -1;
        if (i < t1) {
            t = static_cast<uint64_t>(col_tile[i]);
            r = col_rb[i];
        }
    }
    __device__ __forceinline__ uint4 words(uint64_t t, int &r) const {
        if (t < n_tiles && static_cast<unsigned>(r) < static_cast<unsigned>(nrb)) {
            uint4 x = *reinterpret_cast<const uint4 *>(tiles + t * 128 + (31 - lane) * 4);
            if constexpr (NODES) {
                const uint32_t nb = nbr ? nbr[r] : 0xffffffffu;   // r < S32(n) <= S128(n) * 4
                const uint32_t on = (nb >> lane) & 1u ? 0xffffffffu : 0u;
                x = make_uint4(x.x & rw.x & on, x.y & rw.y & on, x.z & rw.z & on, x.w & rw.w & on);
            }
            return x;
        }
        r = -1;
        return make_uint4(0, 0, 0, 0);
    }
    __device__ __forceinline__ void start(uint64_t b0) {
        uint64_t tc;
        entry(b0 + s_own, tc, rb);
        entry(b0 + TILED_T_TS + s_own, tn, rbn);
        w = words(tc, rb);
    }
    // this round's tile as masks [tile column][staged tile] and its row block; then the next round's loads
    __device__ __forceinline__ void stage(uint64_t base, uint32_t *mk, int *srb) {
        uint32_t v[4] = {w.x, w.y, w.z, w.w};
        tiled_t_transpose(v, lane);
#pragma unroll
        for (int k = 0; k < 4; ++k) mk[(k * 32 + 31 - lane) * TILED_T_TS + s_own] = v[k];
        if (lane == 0) srb[s_own] = rb;
        rb = rbn;
        w = words(tn, rb);
        entry(base + 2 * TILED_T_TS + s_own, tn, rbn);
    }
};
using TiledAttStager = TiledAttStagerOf<false>;

template <int CPL, bool BWD, class... Drop>
__global__ __launch_bounds__(256) void k_tiled_att_f32_t(const int64_t *__restrict__ col_ptr, const int64_t *__restrict__ col_tile,
                                                         const int32_t *__restrict__ col_rb, const uint32_t *__restrict__ tiles,
                                                         uint64_t n_tiles, int n, const float *__restrict__ X, int N, TiledAtt att,
                                                         float *__restrict__ m_out, float *__restrict__ inv_out,
                                                         float *__restrict__ out, Drop... drop) {
    constexpr int LPR = 16, G = 256 / LPR, TS = TILED_T_TS;
    static_assert(TS == 8, "an output row reads its 8 masks of a round as two uint4");
    constexpr int W = LPR * CPL;   // output columns per workgroup
    __shared__ __attribute__((aligned(16))) uint32_t mk[128 * TS];   // [tile column][staged tile]
    __shared__ int srb[TS];
    __shared__ float acc[128 * W];
    __shared__ float dn[BWD ? 1 : 128];
    __shared__ int lists[G][TILED_F32_CAP];
    const int q = blockIdx.x, tid = threadIdx.x;
    const int g = tid / LPR, l = tid % LPR, c0 = blockIdx.y * W + l;
    int *list = lists[g];
    for (int j = g; j < 128; j += G) {
#pragma unroll
        for (int cc = 0; cc < CPL; ++cc) acc[j * W + cc * LPR + l] = 0.0f;
        if constexpr (!BWD)
            if (l == 0) dn[j] = 0.0f;
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
            const float po = att.own[self];
            float mo = 0.0f, den = 0.0f;
            if constexpr (!BWD) {
                mo = tiled_att_shift(po, att.shift[self], att.slope);
                den = dn[j];
            }
            float s[CPL];
#pragma unroll
            for (int cc = 0; cc < CPL; ++cc) s[cc] = acc[j * W + cc * LPR + l];
            int cnt = 0;
#pragma unroll
            for (int st = 0; st < TS; ++st)
                if (m[st]) tiled_att_decode<LPR, CPL, BWD>(m[st], srb[st] * 32, n, s, den, list, cnt, X, N, c0, att, po, mo, tiled_drop_for(self, drop)...);
            tiled_att_add_rows<LPR, CPL, BWD>(s, den, list, cnt, X, N, c0, att, po, mo);
#pragma unroll
            for (int cc = 0; cc < CPL; ++cc) acc[j * W + cc * LPR + l] = s[cc];
            if constexpr (!BWD)
                if (l == 0) dn[j] = den;
        }
        __syncthreads();
    }

    for (int j = g; j < 128; j += G) {
        const int row = q * 128 + j;
        if (row >= n) break;
        float inv = 1.0f;
        if constexpr (!BWD) {
            const float den = dn[j];
            inv = den > 0.0f ? __fdiv_rn(1.0f, den) : 0.0f;
            if (blockIdx.y == 0 && l == 0) {
                m_out[row] = tiled_att_shift(att.own[row], att.shift[row], att.slope);
                inv_out[row] = inv;
            }
        }
#pragma unroll
        for (int cc = 0; cc < CPL; ++cc) {
            const int c = c0 + cc * LPR;
            const float s = acc[j * W + cc * LPR + l];
            if (c < N) out[static_cast<uint64_t>(row) * N + c] = BWD ? s : tiled_att_mul(s, inv);
        }
    }
}

// the score gradient on the column view: tiled_att_grad_rows with a wave per output row, the running sum of every row in LDS between
// rounds (written and read by lane 0 of the row's wave; every lane of the wave computes the same word)
template <bool REG, bool NBR_OWNS, class... Drop>
__global__ __launch_bounds__(256) void k_tiled_att_grad_t(const int64_t *__restrict__ col_ptr, const int64_t *__restrict__ col_tile,
                                                          const int32_t *__restrict__ col_rb, const uint32_t *__restrict__ tiles,
                                                          uint64_t n_tiles, int n, const float *__restrict__ A,
                                                          const float *__restrict__ B, int N, TiledAtt att, float *__restrict__ out,
                                                          Drop... drop) {
    constexpr int G = 4, TS = TILED_T_TS;
    static_assert(TS == 8, "an output row reads its 8 masks of a round as two uint4");
    __shared__ __attribute__((aligned(16))) uint32_t mk[128 * TS];   // [tile column][staged tile]
    __shared__ int srb[TS];
    __shared__ float acc[128];
    __shared__ int lists[G][TILED_F32_CAP];
    const int q = blockIdx.x, tid = threadIdx.x;
    const int g = __builtin_amdgcn_readfirstlane(tid / 64), l = tid % 64;
    int *list = lists[g];
    if (tid < 128) acc[tid] = 0.0f;

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
            const float po = att.own[self];
            float mo = 0.0f, io = 0.0f, Do = 0.0f, own[4];
            if constexpr (!NBR_OWNS) {
                mo = att.shift[self];
                io = att.inv[self];
                Do = att.D[self];
            }
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) own[cc] = REG && l + cc * 64 < N ? Arow[l + cc * 64] : 0.0f;
            float s = acc[j];
            int cnt = 0;
#pragma unroll
            for (int st = 0; st < TS; ++st)
                if (m[st]) tiled_att_grad_decode<REG, NBR_OWNS>(m[st], srb[st] * 32, n, s, own, Arow, list, cnt, B, N, l, att, po, mo, io, Do, tiled_drop_for(self, drop)...);
            tiled_att_grad_rows<REG, NBR_OWNS>(s, own, Arow, list, cnt, B, N, l, att, po, mo, io, Do);
            if (l == 0) acc[j] = s;
        }
        __syncthreads();
    }
    __syncthreads();
    if (tid < 128 && q * 128 + tid < n) out[q * 128 + tid] = acc[tid];
}

// ---- the launchers of k_tiled_att_f32_t (the shapes are the transposed float product's: tiled_col_width_switch) and k_tiled_att_grad_t:
// tiled_att_f32_launch and tiled_att_grad_launch on the column view ------------------------------------------------------------------------
template <bool BWD, class... Drop>
int tiled_att_f32_launch(const TiledColIndex &ix, const uint32_t *tiles, int64_t n_tiles, int n, const float *X, int N, const TiledAtt &att,
                         float *m, float *inv, float *out, hipStream_t st, Drop... drop) {
    tiled_col_width_switch(N, [&](auto cpl) {
        constexpr int CPL = decltype(cpl)::value;
        hipLaunchKernelGGL((k_tiled_att_f32_t<CPL, BWD, Drop...>), tiled_col_grid(n, N, 16 * CPL), dim3(256), 0, st, ix.col_ptr, ix.col_tile,
                           ix.col_rb, tiles, static_cast<uint64_t>(n_tiles), n, X, N, att, m, inv, out, drop...);
    });
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

// REG as on the row view (tests/tiled_attn_model.py, ATT_GRAD_VARIANTS)
template <bool NBR_OWNS, class... Drop>
int tiled_att_grad_launch(const TiledColIndex &ix, const uint32_t *tiles, int64_t n_tiles, int n, const float *A, const float *B, int N,
                          const TiledAtt &att, float *out, hipStream_t st, Drop... drop) {
    const dim3 block(256), grid(step128(n));
    const uint64_t nt = static_cast<uint64_t>(n_tiles);
    if (N <= 256)
        hipLaunchKernelGGL((k_tiled_att_grad_t<true, NBR_OWNS, Drop...>), grid, block, 0, st, ix.col_ptr, ix.col_tile, ix.col_rb, tiles, nt, n,
                           A, B, N, att, out, drop...);
    else
        hipLaunchKernelGGL((k_tiled_att_grad_t<false, NBR_OWNS, Drop...>), grid, block, 0, st, ix.col_ptr, ix.col_tile, ix.col_rb, tiles, nt, n,
                           A, B, N, att, out, drop...);
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

}  // namespace
