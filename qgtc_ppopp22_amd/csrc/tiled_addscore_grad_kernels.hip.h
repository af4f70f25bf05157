// tiled_addscore_grad_kernels.hip.h — part of libqgtc_hip.so (included by qgtc_tiled_addscore_grad.hip and, with
// QGTC_TILED_ADDSCORE_T defined and after tiled_t_kernels.hip.h, by qgtc_tiled_addscore_grad_t.hip; both include
// tiled_float_kernels.hip.h and tiled_attn_kernels.hip.h first): the two folds of the additive score's backward,
//     FD[o, c] = fold over o's neighbours k, ascending, of fl(acc + (u > 0 ? g : fl(a * g))),   d_own[o, c] = fl(att[c] * FD[o, c])
//     FV[o, c] = fold over o's neighbours k, ascending, of fl(acc + fl(g * L(u))),              P[o, c] = FV[o, c]
// with u = fl(own[o, c] + nbr[k, c]) and g = g[slot(o, k) * H + c / d] (include/qgtc_addscore.h). The kernels are
// k_tiled_mm_f32_heads and k_tiled_mm_f32_t_heads of tiled_heads_mm_kernels.hip.h with the adder's term replaced: the walk, the queues of
// neighbours and slots, the slot arithmetic (TiledEdgeRow / TiledEdgeCol of tiled_edge.hip.h, used as they are), the width classes and
// the batched loads are theirs. A lane keeps own[o, c] and att[c] of its columns in registers and one accumulator per column and
// output; WD / WP say which outputs the launch writes, and the other fold is not computed.
#pragma once

namespace {

// the head of each of the lane's columns c0 + cc * LPR (a column past N is never stored: it takes head 0's gradient)
template <int LPR, int CPL>
__device__ __forceinline__ void tiled_addg_heads_of(int (&hh)[CPL], int c0, int N, int H) {
    const int d = N / H;
#pragma unroll
    for (int cc = 0; cc < CPL; ++cc) hh[cc] = c0 + cc * LPR < N ? (c0 + cc * LPR) / d : 0;
}

__device__ __forceinline__ float tiled_addg_add(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}

// the two folds over the queue's entries j = 0 .. cnt-1, IN THAT ORDER; the loads of TILED_F32_AHEAD neighbours, rows and gradients,
// are issued together. A slot outside [0, n_values) - a foreign index - reads nothing and counts as 0.
template <int LPR, int CPL, bool WD, bool WP>
__device__ __forceinline__ void tiled_addg_rows(float (&fd)[CPL], float (&fv)[CPL], const float (&own)[CPL], const int *list,
                                                const TiledEdgeQueue &e, int cnt, const float *__restrict__ X, int N, int c0, int H,
                                                const int (&hh)[CPL], float slope) {
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
                for (int cc = 0; cc < CPL; ++cc) {
                    const float uu = tiled_addg_add(own[cc], x[u][cc]);
                    if constexpr (WD) fd[cc] = tiled_addg_add(fd[cc], uu > 0.0f ? w[u][cc] : tiled_att_mul(slope, w[u][cc]));
                    if constexpr (WP) fv[cc] = tiled_f32_mul_add(fv[cc], w[u][cc], tiled_att_lrelu(uu, slope));
                }
            }
    }
}

// tiled_heads_decode with the two folds; E is TiledEdgeRow or TiledEdgeCol
template <int LPR, int CPL, bool WD, bool WP, class E>
__device__ __forceinline__ void tiled_addg_decode(uint32_t m, int base, int n, float (&fd)[CPL], float (&fv)[CPL], const float (&own)[CPL],
                                                  int *list, int &cnt, const float *__restrict__ X, int N, int c0, const E &e, int H,
                                                  const int (&hh)[CPL], float slope) {
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
                tiled_addg_rows<LPR, CPL, WD, WP>(fd, fv, own, list, e, cnt, X, N, c0, H, hh, slope);
                cnt = 0;
            }
        }
    }
}

// what the kernels take beside the walk's arguments
struct TiledAddGrad {
    const float *own, *nbr, *att;
    float slope;
    float *d_own, *P;
};

#ifndef QGTC_TILED_ADDSCORE_T
// ---- the row view: the walk of k_tiled_mm_f32_heads ---------------------------------------------------------------------------------------
template <int LPR, int CPL, bool WD, bool WP>
__global__ __launch_bounds__(256) void k_tiled_addscore_grad(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ kquad,
                                                             const uint32_t *__restrict__ tiles, uint64_t n_tiles, int n, int N,
                                                             TiledAddGrad ag, TiledEdge ed, int H) {
    constexpr int G = 256 / LPR, RPG = 32 / G;   // row groups per workgroup, rows per group
    __shared__ int lists[G][RPG][TILED_F32_CAP];
    __shared__ int edge_slots[G][RPG][TILED_F32_CAP];
    int *slots = &edge_slots[threadIdx.x / LPR][0][0];
    int vp = 0, vr = 0;   // val_ptr of the tile being decoded; lane l < RPG: val_row of its row of that tile
    const int rb = blockIdx.x, tid = threadIdx.x;
    const int g = LPR == 64 ? __builtin_amdgcn_readfirstlane(tid / LPR) : tid / LPR;
    const int l = tid % LPR, c0 = blockIdx.y * (LPR * CPL) + l;
    const int nq = step128(n);
    const float *__restrict__ X = ag.nbr;
    int hh[CPL];
    tiled_addg_heads_of<LPR, CPL>(hh, c0, N, H);

    uint64_t t0 = 0, t1 = 0;
    if (n_tiles != 0) {
        t0 = static_cast<uint64_t>(row_ptr[rb]);
        t1 = static_cast<uint64_t>(row_ptr[rb + 1]);
        t1 = t1 < n_tiles ? t1 : n_tiles;
    }
    float fd[RPG][CPL], fv[RPG][CPL], own[RPG][CPL];
    int cnt[RPG];
#pragma unroll
    for (int ri = 0; ri < RPG; ++ri) {
        cnt[ri] = 0;
        const int row = rb * 32 + g * RPG + ri;
#pragma unroll
        for (int cc = 0; cc < CPL; ++cc) {
            fd[ri][cc] = fv[ri][cc] = 0.0f;
            own[ri][cc] = row < n && c0 + cc * LPR < N ? ag.own[static_cast<uint64_t>(row) * N + c0 + cc * LPR] : 0.0f;
        }
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
                    tiled_addg_decode<LPR, CPL, WD, WP>(wk, q * 128 + k * 32, n, fd[ri], fv[ri], own[ri], lists[g][ri], cnt[ri], X, N, c0,
                                                        tiled_edge_for(TiledEdgeAtRow{slots + ri * TILED_F32_CAP, sb}, ed), H, hh, ag.slope);
                    sb += __builtin_popcount(wk);
                }
            }
        }
        a = an;
        q = qn;
        vp = vpn;
        vr = vrn;
    }
    float at[CPL];
#pragma unroll
    for (int cc = 0; cc < CPL; ++cc) at[cc] = WD && c0 + cc * LPR < N ? ag.att[c0 + cc * LPR] : 0.0f;
#pragma unroll
    for (int ri = 0; ri < RPG; ++ri) {
        tiled_addg_rows<LPR, CPL, WD, WP>(fd[ri], fv[ri], own[ri], lists[g][ri], tiled_edge_for(TiledEdgeAtFlush{slots + ri * TILED_F32_CAP}, ed),
                                          cnt[ri], X, N, c0, H, hh, ag.slope);
        const int row = rb * 32 + g * RPG + ri;
        if (row < n) {
#pragma unroll
            for (int cc = 0; cc < CPL; ++cc) {
                const int c = c0 + cc * LPR;
                if (c < N) {
                    if constexpr (WD) ag.d_own[static_cast<uint64_t>(row) * N + c] = tiled_att_mul(at[cc], fd[ri][cc]);
                    if constexpr (WP) ag.P[static_cast<uint64_t>(row) * N + c] = fv[ri][cc];
                }
            }
        }
    }
}

template <bool WD, bool WP>
int tiled_addscore_grad_launch(const TiledRowIndex &ix, const uint32_t *tiles, int64_t n_tiles, int n, int N, const TiledAddGrad &ag,
                               hipStream_t st, const TiledEdge &ed, int H) {
    tiled_row_width_switch(N, [&](auto lpr, auto cpl) {
        constexpr int LPR = decltype(lpr)::value, CPL = decltype(cpl)::value;
        hipLaunchKernelGGL((k_tiled_addscore_grad<LPR, CPL, WD, WP>), tiled_row_grid(n, N, LPR * CPL), dim3(256), 0, st, ix.row_ptr, ix.kquad,
                           tiles, static_cast<uint64_t>(n_tiles), n, N, ag, ed, H);
    });
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

#else
// ---- the column view: the walk of k_tiled_mm_f32_t_heads ----------------------------------------------------------------------------------
// The accumulators of a workgroup's 128 output rows live in LDS between the rounds, one array per output the launch writes, so a launch
// that writes both takes 32 columns a workgroup at the most (the extremum's limit, for the same reason: two words of state a column).
template <int LPR, int CPL, bool WD, bool WP>
__global__ __launch_bounds__(256) void k_tiled_addscore_grad_t(const int64_t *__restrict__ col_ptr, const int64_t *__restrict__ col_tile,
                                                               const int32_t *__restrict__ col_rb, const uint32_t *__restrict__ tiles,
                                                               uint64_t n_tiles, int n, int N, TiledAddGrad ag, TiledEdge ed, int H) {
    constexpr int G = 256 / LPR, TS = TILED_T_TS;
    static_assert(TS == 8, "an output row reads its 8 masks of a round as two uint4");
    __shared__ __attribute__((aligned(16))) uint32_t mk[128 * TS];   // [tile column][staged tile]
    __shared__ int srb[TS];
    constexpr int W = LPR * CPL;   // output columns per workgroup
    __shared__ float acc_d[WD ? 128 * W : 1], acc_v[WP ? 128 * W : 1];
    __shared__ int lists[G][TILED_F32_CAP];
    __shared__ int edge_slots[G][TILED_F32_CAP], evr[TS * 32], evp[TS];
    __shared__ __attribute__((aligned(16))) uint32_t raw[TS * 32 * 4];
    int *slots = edge_slots[threadIdx.x / LPR];
    const int q = blockIdx.x, tid = threadIdx.x;
    const int g = tid / LPR;
    const int l = tid % LPR, c0 = blockIdx.y * W + l;
    const int nrb = (n + 31) / 32;
    const float *__restrict__ X = ag.nbr;
    int *list = lists[g];
    int hh[CPL];
    tiled_addg_heads_of<LPR, CPL>(hh, c0, N, H);
    for (int j = g; j < 128; j += G)
#pragma unroll
        for (int cc = 0; cc < CPL; ++cc) {
            if constexpr (WD) acc_d[j * W + cc * LPR + l] = 0.0f;
            if constexpr (WP) acc_v[j * W + cc * LPR + l] = 0.0f;
        }

    const int lane = tid & 31, s_own = tid >> 5;   // transposer role: half-wave s of the workgroup stages tile base + s
    uint64_t b0 = 0, t1 = 0;
    if (n_tiles != 0) {
        b0 = static_cast<uint64_t>(col_ptr[q]);
        t1 = static_cast<uint64_t>(col_ptr[q + 1]);
        t1 = t1 < n_tiles ? t1 : n_tiles;
    }
    uint4 w = make_uint4(0, 0, 0, 0);
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
            float fd[CPL], fv[CPL], own[CPL];
#pragma unroll
            for (int cc = 0; cc < CPL; ++cc) {
                fd[cc] = fv[cc] = 0.0f;
                if constexpr (WD) fd[cc] = acc_d[j * W + cc * LPR + l];
                if constexpr (WP) fv[cc] = acc_v[j * W + cc * LPR + l];
                own[cc] = c0 + cc * LPR < N ? ag.own[static_cast<uint64_t>(q * 128 + j) * N + c0 + cc * LPR] : 0.0f;
            }
            int cnt = 0;
#pragma unroll
            for (int st = 0; st < TS; ++st)
                if (m[st])
                    tiled_addg_decode<LPR, CPL, WD, WP>(m[st], srb[st] * 32, n, fd, fv, own, list, cnt, X, N, c0,
                                                        tiled_edge_for(TiledEdgeAtCol{slots, raw + st * 128, evr + st * 32, evp[st], j}, ed), H, hh,
                                                        ag.slope);
            tiled_addg_rows<LPR, CPL, WD, WP>(fd, fv, own, list, tiled_edge_for(TiledEdgeAtFlush{slots}, ed), cnt, X, N, c0, H, hh, ag.slope);
#pragma unroll
            for (int cc = 0; cc < CPL; ++cc) {
                if constexpr (WD) acc_d[j * W + cc * LPR + l] = fd[cc];
                if constexpr (WP) acc_v[j * W + cc * LPR + l] = fv[cc];
            }
        }
        __syncthreads();
    }

    float at[CPL];
#pragma unroll
    for (int cc = 0; cc < CPL; ++cc) at[cc] = WD && c0 + cc * LPR < N ? ag.att[c0 + cc * LPR] : 0.0f;
    for (int j = g; j < 128; j += G) {
        const int row = q * 128 + j;
        if (row >= n) break;
#pragma unroll
        for (int cc = 0; cc < CPL; ++cc) {
            const int c = c0 + cc * LPR;
            if (c < N) {
                if constexpr (WD) ag.d_own[static_cast<uint64_t>(row) * N + c] = tiled_att_mul(at[cc], acc_d[j * W + cc * LPR + l]);
                if constexpr (WP) ag.P[static_cast<uint64_t>(row) * N + c] = acc_v[j * W + cc * LPR + l];
            }
        }
    }
}

template <bool WD, bool WP>
int tiled_addscore_grad_launch(const TiledColIndex &ix, const uint32_t *tiles, int64_t n_tiles, int n, int N, const TiledAddGrad &ag,
                               hipStream_t st, const TiledEdge &ed, int H) {
    tiled_col_width_switch<(WD && WP) ? 32 : 64>(N, [&](auto cpl) {
        constexpr int CPL = decltype(cpl)::value;
        hipLaunchKernelGGL((k_tiled_addscore_grad_t<16, CPL, WD, WP>), tiled_col_grid(n, N, 16 * CPL), dim3(256), 0, st, ix.col_ptr,
                           ix.col_tile, ix.col_rb, tiles, static_cast<uint64_t>(n_tiles), n, N, ag, ed, H);
    });
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}
#endif

// the entry of either view after its name: the refusals of the weighted sum with heads in its order, then the score's own
template <class Index>
int tiled_addscore_grad_entry(const Index &ix, const uint32_t *tiles, int64_t n_tiles, int n, const float *own, const float *nbr,
                              size_t x_elems, int N, const float *att, size_t att_elems, float slope, float *d_own, float *P,
                              size_t out_elems, const int64_t *val_ptr, const int16_t *val_row, const float *g, size_t n_values,
                              int heads, void *stream) {
    const float *some_out = d_own ? d_own : P;
    int rc = tiled_edge_rc(tiled_f32_args_ok(ix.ok(), tiles, n_tiles, n, own, x_elems, N, nullptr, some_out, out_elems, g),
                           n_tiles > 0 && !g ? QGTC_EINVAL : tiled_edge_index_ok(val_ptr, val_row, n_tiles, n_values));
    int more = QGTC_OK;
    if (!nbr || !att || !(slope >= 0.0f && slope <= 1.0f) || heads < 1 || (N >= 1 && N % heads != 0)) more = QGTC_EINVAL;
    else if (!aligned4(nbr) || !aligned4(att) || !aligned4(d_own) || !aligned4(P)) more = QGTC_EALIGN;
    else if (N >= 1 && att_elems < static_cast<size_t>(N)) more = QGTC_ESIZE;
    rc = tiled_edge_rc(rc, more);
    if (rc != QGTC_OK) return rc;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (!n_tiles || !n_values) {   // no cell: every fold is its +0
        const size_t bytes = static_cast<size_t>(n) * static_cast<size_t>(N) * sizeof(float);
        if (d_own) FILL_TRY(d_own, 0, bytes, st);   // the library's fill kernel: it replays in a captured graph
        if (P) FILL_TRY(P, 0, bytes, st);
        return QGTC_OK;
    }
    const TiledEdge ed{val_ptr, val_row, g, static_cast<int>(n_values)};
    const TiledAddGrad ag{own, nbr, att, slope, d_own, P};
    if (d_own && P) return tiled_addscore_grad_launch<true, true>(ix, tiles, n_tiles, n, N, ag, st, ed, heads);
    if (d_own) return tiled_addscore_grad_launch<true, false>(ix, tiles, n_tiles, n, N, ag, st, ed, heads);
    return tiled_addscore_grad_launch<false, true>(ix, tiles, n_tiles, n, N, ag, st, ed, heads);
}

}  // namespace
