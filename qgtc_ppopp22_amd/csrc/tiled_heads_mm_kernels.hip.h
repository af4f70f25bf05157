// tiled_heads_mm_kernels.hip.h — part of libqgtc_hip.so (included by qgtc_tiled_float_edge_heads.hip and, with
// QGTC_TILED_HEADS_T defined and after tiled_t_kernels.hip.h, by qgtc_tiled_float_t_edge_heads.hip; both include
// tiled_float_kernels.hip.h first): the weighted sum with one weight per stored cell AND HEAD,
//     out[i, c] = row_scale[i] . fold over i's neighbours j, ascending, of fl(acc + fl(values[slot(i, j) * H + c / d] * X[j, c])),
// d = N / H (include/qgtc_heads.h). The operations and their order are those of the kernels whose pack ends
// in TiledEdge (tiled_float_kernels.hip.h, tiled_float_t_kernels.hip.h): the walk, the queues of neighbours and slots, the slot
// arithmetic (TiledEdgeRow / TiledEdgeCol of tiled_edge.hip.h, used as they are) and one unfused multiply and add a term. Only the
// weight's address depends on the lane's column, so the adder loads a weight per column it owns instead of one per neighbour. These
// are kernels of their own: no instantiation of the shared templates changes.
#pragma once

namespace {

// the head of each of the lane's columns c0 + cc * LPR (a column past N is never stored: it takes head 0's weight)
template <int LPR, int CPL>
__device__ __forceinline__ void tiled_heads_of(int (&hh)[CPL], int c0, int N, int H) {
    const int d = N / H;
#pragma unroll
    for (int cc = 0; cc < CPL; ++cc) hh[cc] = c0 + cc * LPR < N ? (c0 + cc * LPR) / d : 0;
}

// tiled_f32_add_rows with the edge values of H heads: s[cc] = fl(s[cc] + fl(values[slots[j] * H + hh[cc]] * X[list[j], c0 + cc * LPR]))
// for j = 0 .. cnt-1, IN THAT ORDER; the loads of TILED_F32_AHEAD neighbours, rows and weights, are issued together. A slot outside
// [0, n_values) - a foreign index - reads nothing and counts as 0.
template <int LPR, int CPL>
__device__ __forceinline__ void tiled_heads_add_rows(float (&s)[CPL], const int *list, const TiledEdgeQueue &e, int cnt,
                                                     const float *__restrict__ X, int N, int c0, int H, const int (&hh)[CPL]) {
#pragma nounroll
    for (int j = 0; j < cnt; j += TILED_F32_AHEAD) {
        float x[TILED_F32_AHEAD][CPL], w[TILED_F32_AHEAD][CPL];
#pragma unroll
        for (int u = 0; u < TILED_F32_AHEAD; ++u) {
            const int i = j + u < cnt ? j + u : cnt - 1;
            const int v = list[i], sl = e.slots[i];
            const float *__restrict__ row = X + static_cast<uint64_t>(v) * N;
            const bool ok = static_cast<unsigned>(sl) < static_cast<unsigned>(e.n_values);
            const float *__restrict__ wr = e.values + static_cast<uint64_t>(ok ? sl : 0) * H;
#pragma unroll
            for (int cc = 0; cc < CPL; ++cc) {
                x[u][cc] = c0 + cc * LPR < N ? row[c0 + cc * LPR] : 0.0f;
                w[u][cc] = ok ? wr[hh[cc]] : 0.0f;
            }
        }
#pragma unroll
        for (int u = 0; u < TILED_F32_AHEAD; ++u)
            if (j + u < cnt) {
#pragma unroll
                for (int cc = 0; cc < CPL; ++cc) s[cc] = tiled_f32_mul_add(s[cc], w[u][cc], x[u][cc]);
            }
    }
}

// tiled_f32_decode with the edge values of H heads; E is TiledEdgeRow or TiledEdgeCol
template <int LPR, int CPL, class E>
__device__ __forceinline__ void tiled_heads_decode(uint32_t m, int base, int n, float (&s)[CPL], int *list, int &cnt,
                                                   const float *__restrict__ X, int N, int c0, const E &e, int H, const int (&hh)[CPL]) {
    int k = 0;   // the set bits of the word consumed so far
    while (m) {
        const int b = __builtin_clz(m);
        m &= ~(0x80000000u >> b);
        const int v = base + b;
        ++k;
        if (v < n) {
            e.slots[cnt] = e.slot(b, k - 1);
            list[cnt++] = v;
            if (cnt == TILED_F32_CAP) {
                tiled_heads_add_rows<LPR, CPL>(s, list, e, cnt, X, N, c0, H, hh);
                cnt = 0;
            }
        }
    }
}

#ifndef QGTC_TILED_HEADS_T
// ---- the row view: k_tiled_mm_f32 with its pack ending in TiledEdge, the weight taken per column ------------------------------------------
template <int LPR, int CPL, bool SCALED>
__global__ __launch_bounds__(256) void k_tiled_mm_f32_heads(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ kquad,
                                                            const uint32_t *__restrict__ tiles, uint64_t n_tiles, int n,
                                                            const float *__restrict__ X, int N, const float *__restrict__ row_scale,
                                                            float *__restrict__ out, TiledEdge ed, int H) {
    constexpr int G = 256 / LPR, RPG = 32 / G;   // row groups per workgroup, rows per group
    __shared__ int lists[G][RPG][TILED_F32_CAP];
    __shared__ int edge_slots[G][RPG][TILED_F32_CAP];
    int *slots = &edge_slots[threadIdx.x / LPR][0][0];
    int vp = 0, vr = 0;   // val_ptr of the tile being decoded; lane l < RPG: val_row of its row of that tile
    const int rb = blockIdx.x, tid = threadIdx.x;
    const int g = LPR == 64 ? __builtin_amdgcn_readfirstlane(tid / LPR) : tid / LPR;
    const int l = tid % LPR, c0 = blockIdx.y * (LPR * CPL) + l;
    const int nq = step128(n);
    int hh[CPL];
    tiled_heads_of<LPR, CPL>(hh, c0, N, H);

    uint64_t t0 = 0, t1 = 0;   // an adjacency without tiles may come without row_ptr
    if (n_tiles != 0) {
        t0 = static_cast<uint64_t>(row_ptr[rb]);
        t1 = static_cast<uint64_t>(row_ptr[rb + 1]);
        t1 = t1 < n_tiles ? t1 : n_tiles;
    }
    float s[RPG][CPL];
    int cnt[RPG];
#pragma unroll
    for (int ri = 0; ri < RPG; ++ri) {
        cnt[ri] = 0;
#pragma unroll
        for (int cc = 0; cc < CPL; ++cc) s[ri][cc] = 0.0f;
    }
    const uint32_t *mine = tiles + (g * RPG + (l < RPG ? l : 0)) * 4;   // lane l < RPG: row g * RPG + l of every tile
    uint4 a = make_uint4(0, 0, 0, 0);
    int q = -1;
    if (t0 < t1) {
        q = kquad[t0];
        if (l < RPG) a = *reinterpret_cast<const uint4 *>(mine + t0 * 128);
        vp = static_cast<int>(ed.val_ptr[t0]);
        if (l < RPG) vr = ed.val_row[t0 * 32 + g * RPG + l];
    }
    for (uint64_t t = t0; t < t1; ++t) {
        uint4 an = make_uint4(0, 0, 0, 0);
        int qn = -1, vpn = 0, vrn = 0;
        if (t + 1 < t1) {
            qn = kquad[t + 1];
            if (l < RPG) an = *reinterpret_cast<const uint4 *>(mine + (t + 1) * 128);
            vpn = static_cast<int>(ed.val_ptr[t + 1]);
            if (l < RPG) vrn = ed.val_row[(t + 1) * 32 + g * RPG + l];
        }
        if (static_cast<unsigned>(q) < static_cast<unsigned>(nq)) {
            const uint32_t w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
            for (int ri = 0; ri < RPG; ++ri) {
                int sb = vp + static_cast<int>(tiled_f32_bcast<LPR>(static_cast<uint32_t>(vr), ri));   // the slot of the row's next set bit
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t wk = tiled_f32_bcast<LPR>(w[k], ri);
                    tiled_heads_decode<LPR, CPL>(wk, q * 128 + k * 32, n, s[ri], lists[g][ri], cnt[ri], X, N, c0,
                                                 tiled_edge_for(TiledEdgeAtRow{slots + ri * TILED_F32_CAP, sb}, ed), H, hh);
                    sb += __builtin_popcount(wk);
                }
            }
        }
        a = an;
        q = qn;
        vp = vpn;
        vr = vrn;
    }
#pragma unroll
    for (int ri = 0; ri < RPG; ++ri) {
        tiled_heads_add_rows<LPR, CPL>(s[ri], lists[g][ri], tiled_edge_for(TiledEdgeAtFlush{slots + ri * TILED_F32_CAP}, ed), cnt[ri], X, N, c0,
                                       H, hh);
        const int row = rb * 32 + g * RPG + ri;
        if (row < n) {
            float sc = 1.0f;
            if constexpr (SCALED) sc = row_scale[row];
#pragma unroll
            for (int cc = 0; cc < CPL; ++cc) {
                const int c = c0 + cc * LPR;
                if (c < N) out[static_cast<uint64_t>(row) * N + c] = SCALED ? s[ri][cc] * sc : s[ri][cc];
            }
        }
    }
}

template <bool SCALED>
int tiled_mm_f32_heads_launch(const TiledRowIndex &ix, const uint32_t *tiles, int64_t n_tiles, int n, const float *X, int N,
                              const float *row_scale, float *out, hipStream_t st, const TiledEdge &ed, int H) {
    tiled_row_width_switch(N, [&](auto lpr, auto cpl) {
        constexpr int LPR = decltype(lpr)::value, CPL = decltype(cpl)::value;
        hipLaunchKernelGGL((k_tiled_mm_f32_heads<LPR, CPL, SCALED>), tiled_row_grid(n, N, LPR * CPL), dim3(256), 0, st, ix.row_ptr, ix.kquad,
                           tiles, static_cast<uint64_t>(n_tiles), n, X, N, row_scale, out, ed, H);
    });
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

#else
// ---- the column view: k_tiled_mm_f32_t with its pack ending in TiledEdge, the weight taken per column ------------------------------------
template <int LPR, int CPL, bool SCALED>
__global__ __launch_bounds__(256) void k_tiled_mm_f32_t_heads(const int64_t *__restrict__ col_ptr, const int64_t *__restrict__ col_tile,
                                                              const int32_t *__restrict__ col_rb, const uint32_t *__restrict__ tiles,
                                                              uint64_t n_tiles, int n, const float *__restrict__ X, int N,
                                                              const float *__restrict__ row_scale, float *__restrict__ out, TiledEdge ed,
                                                              int H) {
    constexpr int G = 256 / LPR, TS = TILED_T_TS;
    static_assert(TS == 8, "an output row reads its 8 masks of a round as two uint4");
    __shared__ __attribute__((aligned(16))) uint32_t mk[128 * TS];   // [tile column][staged tile]
    __shared__ int srb[TS];
    constexpr int W = LPR * CPL;   // output columns per workgroup
    __shared__ float acc[128 * W];
    __shared__ int lists[G][TILED_F32_CAP];
    // the slots of this row group's queued neighbours; the round's words before the transpose and their val_row, [staged tile][tile
    // row]; the staged tiles' val_ptr
    __shared__ int edge_slots[G][TILED_F32_CAP], evr[TS * 32], evp[TS];
    __shared__ __attribute__((aligned(16))) uint32_t raw[TS * 32 * 4];
    int *slots = edge_slots[threadIdx.x / LPR];
    const int q = blockIdx.x, tid = threadIdx.x;
    const int g = tid / LPR;
    const int l = tid % LPR, c0 = blockIdx.y * W + l;
    const int nrb = (n + 31) / 32;
    int *list = lists[g];
    int hh[CPL];
    tiled_heads_of<LPR, CPL>(hh, c0, N, H);
    for (int j = g; j < 128; j += G)
#pragma unroll
        for (int cc = 0; cc < CPL; ++cc) acc[j * W + cc * LPR + l] = 0.0f;

    const int lane = tid & 31, s_own = tid >> 5;   // transposer role: half-wave s of the workgroup stages tile base + s
    uint64_t b0 = 0, t1 = 0;                       // an adjacency without tiles may come without col_ptr
    if (n_tiles != 0) {
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
        if (t < n_tiles && static_cast<unsigned>(rb) < static_cast<unsigned>(nrb))
            return *reinterpret_cast<const uint4 *>(tiles + t * 128 + (31 - lane) * 4);
        rb = -1;
        return make_uint4(0, 0, 0, 0);
    };
    // val_row of this lane's tile row and the tile's val_ptr, after words() has checked the entry (rb < 0: none)
    int vr = 0, vp = 0;
    auto evals = [&](uint64_t t, int rb) {
        vr = vp = 0;
        if (rb >= 0) {
            vr = ed.val_row[t * 32 + (31 - lane)];
            vp = static_cast<int>(ed.val_ptr[t]);
        }
    };
    uint64_t tn;
    int rb, rbn;
    {
        uint64_t tc;
        entry(b0 + s_own, tc, rb);
        entry(b0 + TS + s_own, tn, rbn);
        w = words(tc, rb);
        evals(tc, rb);
    }
    for (uint64_t base = b0; base < t1; base += TS) {
        {
            uint32_t v[4] = {w.x, w.y, w.z, w.w};
            *reinterpret_cast<uint4 *>(raw + (s_own * 32 + 31 - lane) * 4) = w;
            evr[s_own * 32 + 31 - lane] = vr;
            if (lane == 0) evp[s_own] = vp;
            tiled_t_transpose(v, lane);
#pragma unroll
            for (int k = 0; k < 4; ++k) mk[(k * 32 + 31 - lane) * TS + s_own] = v[k];
            if (lane == 0) srb[s_own] = rb;
            rb = rbn;
            w = words(tn, rb);
            evals(tn, rb);
            entry(base + 2 * TS + s_own, tn, rbn);
        }
        __syncthreads();
        for (int j = g; j < 128; j += G) {
            if (q * 128 + j >= n) break;
            const uint4 ma = *reinterpret_cast<const uint4 *>(mk + j * TS), mb = *reinterpret_cast<const uint4 *>(mk + j * TS + 4);
            const uint32_t m[TS] = {ma.x, ma.y, ma.z, ma.w, mb.x, mb.y, mb.z, mb.w};
            if (!(ma.x | ma.y | ma.z | ma.w | mb.x | mb.y | mb.z | mb.w)) continue;
            float s[CPL];
#pragma unroll
            for (int cc = 0; cc < CPL; ++cc) s[cc] = acc[j * W + cc * LPR + l];
            int cnt = 0;
#pragma unroll
            for (int st = 0; st < TS; ++st)
                if (m[st])
                    tiled_heads_decode<LPR, CPL>(m[st], srb[st] * 32, n, s, list, cnt, X, N, c0,
                                                 tiled_edge_for(TiledEdgeAtCol{slots, raw + st * 128, evr + st * 32, evp[st], j}, ed), H, hh);
            tiled_heads_add_rows<LPR, CPL>(s, list, tiled_edge_for(TiledEdgeAtFlush{slots}, ed), cnt, X, N, c0, H, hh);
#pragma unroll
            for (int cc = 0; cc < CPL; ++cc) acc[j * W + cc * LPR + l] = s[cc];
        }
        __syncthreads();
    }

    for (int j = g; j < 128; j += G) {
        const int row = q * 128 + j;
        if (row >= n) break;
        float sc = 1.0f;
        if constexpr (SCALED) sc = row_scale[row];
#pragma unroll
        for (int cc = 0; cc < CPL; ++cc) {
            const int c = c0 + cc * LPR;
            const float s = acc[j * W + cc * LPR + l];
            if (c < N) out[static_cast<uint64_t>(row) * N + c] = SCALED ? s * sc : s;
        }
    }
}

template <bool SCALED>
int tiled_mm_f32_heads_launch(const TiledColIndex &ix, const uint32_t *tiles, int64_t n_tiles, int n, const float *X, int N,
                              const float *row_scale, float *out, hipStream_t st, const TiledEdge &ed, int H) {
    tiled_col_width_switch(N, [&](auto cpl) {
        constexpr int CPL = decltype(cpl)::value;
        hipLaunchKernelGGL((k_tiled_mm_f32_t_heads<16, CPL, SCALED>), tiled_col_grid(n, N, 16 * CPL), dim3(256), 0, st, ix.col_ptr,
                           ix.col_tile, ix.col_rb, tiles, static_cast<uint64_t>(n_tiles), n, X, N, row_scale, out, ed, H);
    });
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}
#endif

// the entry of either view after its name: the single-head entry's refusals in its order, with heads
template <class Index>
int tiled_mm_f32_heads_entry(const Index &ix, const uint32_t *tiles, int64_t n_tiles, int n, const float *X, size_t x_elems, int N,
                             const float *row_scale, float *out, size_t out_elems, const int64_t *val_ptr, const int16_t *val_row,
                             const float *values, size_t n_values, int heads, void *stream) {
    int rc = tiled_edge_rc(tiled_f32_args_ok(ix.ok(), tiles, n_tiles, n, X, x_elems, N, row_scale, out, out_elems, values),
                           n_tiles > 0 && !values ? QGTC_EINVAL : tiled_edge_index_ok(val_ptr, val_row, n_tiles, n_values));
    if (heads < 1 || (N >= 1 && N % heads != 0)) rc = QGTC_EINVAL;
    if (rc != QGTC_OK) return rc;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const TiledEdge ed{val_ptr, val_row, values, static_cast<int>(n_values)};
    return row_scale ? tiled_mm_f32_heads_launch<true>(ix, tiles, n_tiles, n, X, N, row_scale, out, st, ed, heads)
                     : tiled_mm_f32_heads_launch<false>(ix, tiles, n_tiles, n, X, N, nullptr, out, st, ed, heads);
}

}  // namespace
