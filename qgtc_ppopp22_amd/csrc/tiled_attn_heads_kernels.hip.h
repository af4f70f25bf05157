// tiled_attn_heads_kernels.hip.h — part of libqgtc_hip.so (included by the qgtc_tiled_attn_heads*.hip units, after
// tiled_float_kernels.hip.h, tiled_max_kernels.hip.h and tiled_attn_kernels.hip.h): the attention product and its three gradients for
// H HEADS in one launch (include/qgtc_attn_heads.h) - the adders, the kernels on the row view, the row dot,
// the shapes, the argument checks and the launchers. tiled_attn_heads_t_kernels.hip.h has the column view.
//
// A node matrix is [n, N] with N = H * d, head h in the columns h * d ..; every per-node vector is [n, H], element node * H + h. The
// walk, the queues, the masks in the trailing pack and every arithmetic function (tiled_att_weight, tiled_att_shift, tiled_f32_mul_add,
// tiled_att_wave_sum) are those of tiled_attn_kernels.hip.h, used as they are: what is new is which head a lane's column belongs to.
//   product   every column's fold and every head's den is the single-head kernel's whatever lane holds it, so a lane takes CPL ADJACENT
//             columns c0 .. c0 + CPL - 1: they share a head whenever CPL divides d, and the lane then computes one weight a neighbour.
//             A lane whose columns straddle two heads computes the second head's weight as well (wave-divergent, rare).
//   gradient  DOT over a head's d columns must be the single-head DOT at N = d ("Why the narrow mapping gives the
//             single-head bits"). narrow, d <= 64: a head is an aligned group of P = next_pow2(d) lanes, 64 / P heads share a register
//             slot, a workgroup holds one slot of heads and blockIdx.y counts the slots; wide, d > 64: a head takes the
//             whole wave, blockIdx.y is the head, its slice of the row stays in 4 slots up to d = 256 and is read again beyond.
// No operation is fused: every function below is under `fp contract(off)` or calls one that is.
#pragma once

namespace {

// the scores and statistics of one launch ([n, H] each, as TiledAtt names them) and the heads' shape
struct TiledAttH {
    TiledAtt a;
    int H, d;
    int lg;   // the score gradient, narrow: log2 of the lanes a head takes
};

// the head of each of the lane's columns c0 + cc (a column past N is never stored: it takes the last head's weight)
template <int CPL>
__device__ __forceinline__ void tiled_atth_heads_of(int (&hh)[CPL], int c0, int N, int d) {
#pragma unroll
    for (int cc = 0; cc < CPL; ++cc) hh[cc] = (c0 + cc < N ? c0 + cc : N - 1) / d;
}

// tiled_att_add_rows per column: s[cc] = fl(s[cc] + fl(w_j[head of cc] * X[list[j], c0 + cc])) for j = 0 .. cnt-1 IN THAT ORDER and, in
// the forward, den[cc] = fl(den[cc] + w_j[head of cc]) - every column carries the den of its head (the same word in all of a head's
// columns). `self` is the output row (below n). The weight is computed once per run of columns with one head.
// ONE (the launcher's choice, CPL > 1): CPL divides d and N and X sits on a CPL-float boundary, so a lane's columns share one head and
// are one aligned vector of a row - one score, one weight and one den add a neighbour, one load a row; the same operations on every
// column as without it.
template <int CPL, bool BWD, bool ONE>
__device__ __forceinline__ void tiled_atth_add_rows(float (&s)[CPL], float (&den)[CPL], const int *list, int cnt,
                                                    const float *__restrict__ X, int N, int c0, const TiledAttH &at,
                                                    const int (&hh)[CPL], int self) {
    static_assert(!ONE || CPL == 2 || CPL == 4, "a lane's vector is two or four floats");
    constexpr int K = ONE ? 1 : CPL;   // the heads a lane looks up
    if (cnt == 0) return;
    const int H = at.H;
    float po[K], mo[K];
#pragma unroll
    for (int cc = 0; cc < K; ++cc) {
        po[cc] = at.a.own[static_cast<uint64_t>(self) * H + hh[cc]];
        mo[cc] = 0.0f;
        if constexpr (!BWD) mo[cc] = tiled_att_shift(po[cc], at.a.shift[static_cast<uint64_t>(self) * H + hh[cc]], at.a.slope);
    }
#pragma nounroll
    for (int j = 0; j < cnt; j += TILED_F32_AHEAD) {
        float x[TILED_F32_AHEAD][CPL], qv[TILED_F32_AHEAD][K];
        [[maybe_unused]] float mv[TILED_F32_AHEAD][K], iv[TILED_F32_AHEAD][K];
        tiled_static_for<TILED_F32_AHEAD>([&](auto u) {
            const int v = list[j + u < cnt ? j + u : cnt - 1];
            const float *__restrict__ row = X + static_cast<uint64_t>(v) * N;
            const uint64_t sv = static_cast<uint64_t>(v) * H;
            if constexpr (ONE && CPL == 4) {
                const float4 t = c0 < N ? *reinterpret_cast<const float4 *>(row + c0) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                x[u][0] = t.x, x[u][1] = t.y, x[u][2] = t.z, x[u][3] = t.w;
            } else if constexpr (ONE) {
                const float2 t = c0 < N ? *reinterpret_cast<const float2 *>(row + c0) : make_float2(0.0f, 0.0f);
                x[u][0] = t.x, x[u][1] = t.y;
            } else {
#pragma unroll
                for (int cc = 0; cc < CPL; ++cc) x[u][cc] = c0 + cc < N ? row[c0 + cc] : 0.0f;
            }
#pragma unroll
            for (int cc = 0; cc < K; ++cc) {
                qv[u][cc] = at.a.nbr[sv + hh[cc]];
                if constexpr (BWD) {
                    mv[u][cc] = at.a.shift[sv + hh[cc]];
                    iv[u][cc] = at.a.inv[sv + hh[cc]];
                }
            }
        });
        tiled_static_for<TILED_F32_AHEAD>([&](auto u) {
            if (j + u < cnt) {
                float w = 0.0f;
#pragma unroll
                for (int cc = 0; cc < CPL; ++cc) {
                    if (cc == 0 || (!ONE && hh[cc] != hh[cc - 1])) {
                        constexpr int kk = 0;
                        const int k = ONE ? kk : cc;
                        if constexpr (BWD) w = tiled_att_weight<true>(po[k], qv[u][k], mv[u][k], iv[u][k], at.a.slope);
                        else w = tiled_att_weight<false>(po[k], qv[u][k], mo[k], 0.0f, at.a.slope);
                    }
                    if constexpr (!BWD)
                        if (!ONE || cc == 0) den[cc] += w;
                    s[cc] = tiled_f32_mul_add(s[cc], w, x[u][cc]);
                }
            }
        });
    }
    if constexpr (ONE && !BWD) {
#pragma unroll
        for (int cc = 1; cc < CPL; ++cc) den[cc] = den[0];   // one head: one den, carried by every column
    }
}

// tiled_att_decode on the adjacent columns (the trailing pack is the single-head kernels': nothing, the edge-dropout mask of
// tiled_drop.hip.h or the node masks of tiled_nodes.hip.h)
template <int CPL, bool BWD, bool ONE, class... Drop>
__device__ __forceinline__ void tiled_atth_decode(uint32_t m, int base, int n, float (&s)[CPL], float (&den)[CPL], int *list, int &cnt,
                                                  const float *__restrict__ X, int N, int c0, const TiledAttH &at, const int (&hh)[CPL],
                                                  int self, Drop... drop) {
    while (m) {
        const int b = __builtin_clz(m);
        m &= ~(0x80000000u >> b);
        const int v = base + b;
        if (v < n && tiled_drop_kept(v, drop...)) {
            list[cnt++] = v;
            if (cnt == TILED_F32_CAP) {
                tiled_atth_add_rows<CPL, BWD, ONE>(s, den, list, cnt, X, N, c0, at, hh, self);
                cnt = 0;
            }
        }
    }
}

// ---- the row view: k_tiled_att_f32 with lane l of a row group on the columns chunk + l * CPL .. + CPL - 1 -------------------------------
//   forward (BWD false)  out[o, c] = fl(s * inv[o, h]), inv = fl(1 / den), 0 for a row without neighbours; the lane that holds a head's
//                        first column also stores m[o, h] and inv[o, h];
//   backward (BWD true)  out[k, c] = s, the weights normalised per term by the neighbour's own statistics of the column's head.
template <int LPR, int CPL, bool BWD, bool ONE, class... Drop>
__global__ __launch_bounds__(256) void k_tiled_att_heads_f32(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ kquad,
                                                             const uint32_t *__restrict__ tiles, uint64_t n_tiles, int n,
                                                             const float *__restrict__ X, int N, TiledAttH at, float *__restrict__ m_out,
                                                             float *__restrict__ inv_out, float *__restrict__ out, Drop... drop) {
    constexpr int G = 256 / LPR, RPG = 32 / G;
    __shared__ int lists[G][RPG][TILED_F32_CAP];
    const int rb = blockIdx.x, tid = threadIdx.x;
    const int g = LPR == 64 ? __builtin_amdgcn_readfirstlane(tid / LPR) : tid / LPR;
    const int l = tid % LPR, c0 = blockIdx.y * (LPR * CPL) + l * CPL;
    const int nq = step128(n);
    int hh[CPL];
    tiled_atth_heads_of<CPL>(hh, c0, N, at.d);

    constexpr bool NODES = tiled_has_nodes<Drop...>();
    [[maybe_unused]] const TiledNodes nodes = tiled_nodes_of(drop...);
    [[maybe_unused]] uint32_t rword = 0;   // the row bitmap's word of this block
    if constexpr (NODES) rword = tiled_nodes_word(nodes.row, rb);

    uint64_t t0 = 0, t1 = 0;   // an adjacency without tiles may come without row_ptr
    bool walk = n_tiles != 0;
    if constexpr (NODES) walk = walk && rword != 0;
    if (walk) {
        t0 = static_cast<uint64_t>(row_ptr[rb]);
        t1 = static_cast<uint64_t>(row_ptr[rb + 1]);
        t1 = t1 < n_tiles ? t1 : n_tiles;
    }
    const int row0 = rb * 32 + g * RPG;
    float s[RPG][CPL], den[RPG][CPL];
    int cnt[RPG];
    tiled_static_for<RPG>([&](auto ri) {
        cnt[ri] = 0;
#pragma unroll
        for (int cc = 0; cc < CPL; ++cc) s[ri][cc] = den[ri][cc] = 0.0f;
    });
    const uint32_t *mine = tiles + (g * RPG + (l < RPG ? l : 0)) * 4;   // lane l < RPG: row g * RPG + l of every tile
    bool loads = l < RPG;
    if constexpr (NODES) loads = loads && tiled_nodes_bit(rword, (g * RPG + l) & 31);
    uint4 a = make_uint4(0, 0, 0, 0);
    [[maybe_unused]] uint4 nb = make_uint4(0, 0, 0, 0), nbn = make_uint4(0, 0, 0, 0);   // the neighbour bitmap's words of k-quad q / qn
    int q = -1;
    if (t0 < t1) {
        q = kquad[t0];
        if (loads) a = *reinterpret_cast<const uint4 *>(mine + t0 * 128);
        if constexpr (NODES)
            if (static_cast<unsigned>(q) < static_cast<unsigned>(nq)) nb = tiled_nodes_quad(nodes.nbr, q);
    }
    for (uint64_t t = t0; t < t1; ++t) {
        uint4 an = make_uint4(0, 0, 0, 0);
        int qn = -1;
        if (t + 1 < t1) {
            qn = kquad[t + 1];
            if (loads) an = *reinterpret_cast<const uint4 *>(mine + (t + 1) * 128);
            if constexpr (NODES)
                if (static_cast<unsigned>(qn) < static_cast<unsigned>(nq)) nbn = tiled_nodes_quad(nodes.nbr, qn);
        }
        bool decode = static_cast<unsigned>(q) < static_cast<unsigned>(nq);
        if constexpr (NODES) decode = decode && (nb.x | nb.y | nb.z | nb.w) != 0;
        if (decode) {
            const uint32_t w[4] = {a.x, a.y, a.z, a.w};
            [[maybe_unused]] const uint32_t nw[4] = {nb.x, nb.y, nb.z, nb.w};
            tiled_static_for<RPG>([&](auto ri) {
                const int row = row0 + ri < n ? row0 + ri : n - 1;   // a row past n walks zero words and stores nothing
                tiled_static_for<4>([&](auto k) {
                    uint32_t mw = tiled_f32_bcast<LPR>(w[k], ri);
                    if constexpr (NODES) mw &= nw[k];
                    tiled_atth_decode<CPL, BWD, ONE>(mw, q * 128 + k * 32, n, s[ri], den[ri], lists[g][ri], cnt[ri], X, N, c0, at, hh, row,
                                                tiled_drop_for(row0 + ri, drop)...);
                });
            });
        }
        a = an;
        q = qn;
        if constexpr (NODES) nb = nbn;
    }
    tiled_static_for<RPG>([&](auto ri) {
        const int row = row0 + ri;
        tiled_atth_add_rows<CPL, BWD, ONE>(s[ri], den[ri], lists[g][ri], cnt[ri], X, N, c0, at, hh, row < n ? row : n - 1);
        if (row < n) {
#pragma unroll
            for (int cc = 0; cc < CPL; ++cc) {
                const int c = c0 + cc;
                if (c < N) {
                    float inv = 1.0f;
                    if constexpr (!BWD) {
                        inv = den[ri][cc] > 0.0f ? __fdiv_rn(1.0f, den[ri][cc]) : 0.0f;
                        if (c % at.d == 0) {
                            const uint64_t sh = static_cast<uint64_t>(row) * at.H + hh[cc];
                            m_out[sh] = tiled_att_shift(at.a.own[sh], at.a.shift[sh], at.a.slope);
                            inv_out[sh] = inv;
                        }
                    }
                    out[static_cast<uint64_t>(row) * N + c] = BWD ? s[ri][cc] : tiled_att_mul(s[ri][cc], inv);
                }
            }
        }
    });
}

// ---- the score gradient ---------------------------------------------------------------------------------------------------------------
// the xor butterfly within aligned groups of 1 << lg lanes, the largest distance first: tiled_att_wave_sum without its stages from
// distance 1 << lg up (there a head's lanes would add the +0 of lanes outside the head)
__device__ __forceinline__ float tiled_atth_group_sum(float t, int lg) {
    for (int h = (1 << lg) >> 1; h >= 1; h >>= 1) t += __shfl_xor(t, h, 64);
    return t;
}

// acc = fl(acc + u), u = fl(alpha * fl(t - D)), times the slope where the edge's e is not positive: the tail of tiled_att_grad_rows
__device__ __forceinline__ void tiled_atth_fold(float &acc, float t, float po, float qv, float m, float inv, float D, float slope) {
#pragma clang fp contract(off)
    const float alpha = tiled_att_weight<true>(po, qv, m, inv, slope);
    float g = tiled_att_mul(alpha, tiled_att_sub(t, D));
    const float e = po + qv;
    if (!(e > 0.0f)) g = slope * g;
    acc = acc + g;
}

// what a lane holds of the heads of its workgroup. Narrow: slot k is the padded column l + 64 (blockIdx.y * NS + k) = head * P + idx,
// column head * d + idx of the matrix when idx < d and the head exists, padding (+0) otherwise. Wide: the head is blockIdx.y and slot
// k its column l + 64 k. `hd` is clamped to an existing head: a padding slot computes on that head's scores and stores nothing.
template <int R, bool WIDE>
struct TiledAttHLane {
    int col[R], hd[WIDE ? 1 : R];
    bool first[WIDE ? 1 : R];   // this lane stores the head's result
    __device__ __forceinline__ void make(const TiledAttH &at, int y, int l) {
        if constexpr (WIDE) {
            hd[0] = y < at.H ? y : at.H - 1;
            first[0] = l == 0 && y < at.H;
#pragma unroll
            for (int k = 0; k < R; ++k) col[k] = y < at.H && l + 64 * k < at.d ? y * at.d + l + 64 * k : -1;
        } else {
#pragma unroll
            for (int k = 0; k < R; ++k) {
                const int pc = l + 64 * (y * R + k), h = pc >> at.lg, idx = pc & ((1 << at.lg) - 1);
                hd[k] = h < at.H ? h : at.H - 1;
                first[k] = idx == 0 && h < at.H;
                col[k] = h < at.H && idx < at.d ? h * at.d + idx : -1;
            }
        }
    }
};

// tiled_att_grad_rows for the heads of the workgroup: acc[k] (narrow: the head of slot k; wide: acc[0], the head) = fl(acc + u) for
// the neighbours list[0 .. cnt) IN THAT ORDER. NS slots hold the out node's row (`a`) and each neighbour's; NS = 0 (wide only) reads
// both again for every neighbour. `self` is the out node (below n).
template <int NS, bool WIDE, bool NBR_OWNS>
__device__ __forceinline__ void tiled_atth_grad_rows(float (&acc)[WIDE ? 1 : NS], const float (&a)[NS ? NS : 1],
                                                     const TiledAttHLane<(NS ? NS : 1), WIDE> &ln, const float *__restrict__ Arow,
                                                     const int *list, int cnt, const float *__restrict__ B, int N, int l,
                                                     const TiledAttH &at, int self) {
    constexpr int R = NS ? NS : 1, S = WIDE ? 1 : NS;   // slots of row data, heads a lane takes part in
    if (cnt == 0) return;
    const int H = at.H;
    float po[S], mo[S], io[S], Do[S];
#pragma unroll
    for (int k = 0; k < S; ++k) {
        const uint64_t sh = static_cast<uint64_t>(self) * H + ln.hd[k];
        po[k] = at.a.own[sh];
        mo[k] = io[k] = Do[k] = 0.0f;
        if constexpr (!NBR_OWNS) {
            mo[k] = at.a.shift[sh];
            io[k] = at.a.inv[sh];
            Do[k] = at.a.D[sh];
        }
    }
#pragma nounroll
    for (int j = 0; j < cnt; j += TILED_F32_AHEAD) {
        [[maybe_unused]] float b[TILED_F32_AHEAD][R];
        float qv[TILED_F32_AHEAD][S];
        int v[TILED_F32_AHEAD];
        [[maybe_unused]] float mv[TILED_F32_AHEAD][S], iv[TILED_F32_AHEAD][S], dv[TILED_F32_AHEAD][S];
        tiled_static_for<TILED_F32_AHEAD>([&](auto u) {
            v[u] = list[j + u < cnt ? j + u : cnt - 1];
            if constexpr (NS != 0) {
                const float *__restrict__ row = B + static_cast<uint64_t>(v[u]) * N;
#pragma unroll
                for (int k = 0; k < R; ++k) b[u][k] = ln.col[k] >= 0 ? row[ln.col[k]] : 0.0f;
            }
#pragma unroll
            for (int k = 0; k < S; ++k) {
                const uint64_t sv = static_cast<uint64_t>(v[u]) * H + ln.hd[k];
                qv[u][k] = at.a.nbr[sv];
                if constexpr (NBR_OWNS) {
                    mv[u][k] = at.a.shift[sv];
                    iv[u][k] = at.a.inv[sv];
                    dv[u][k] = at.a.D[sv];
                }
            }
        });
        tiled_static_for<TILED_F32_AHEAD>([&](auto u) {
            if (j + u < cnt) {
                if constexpr (WIDE) {
                    float t = 0.0f;
                    if constexpr (NS != 0) {
#pragma unroll
                        for (int k = 0; k < R; ++k) t = tiled_f32_mul_add(t, a[k], b[u][k]);   // past d: + fl(0 * 0), the same bits
                    } else {
                        const float *__restrict__ ar = Arow + ln.hd[0] * at.d;
                        const float *__restrict__ br = B + static_cast<uint64_t>(v[u]) * N + ln.hd[0] * at.d;
                        for (int c = l; c < at.d; c += 64) t = tiled_f32_mul_add(t, ar[c], br[c]);
                    }
                    t = tiled_att_wave_sum(t);
                    tiled_atth_fold(acc[0], t, po[0], qv[u][0], NBR_OWNS ? mv[u][0] : mo[0], NBR_OWNS ? iv[u][0] : io[0],
                                    NBR_OWNS ? dv[u][0] : Do[0], at.a.slope);
                } else {
#pragma unroll
                    for (int k = 0; k < S; ++k) {
                        const float t = tiled_atth_group_sum(tiled_f32_mul_add(0.0f, a[k], b[u][k]), at.lg);
                        tiled_atth_fold(acc[k], t, po[k], qv[u][k], NBR_OWNS ? mv[u][k] : mo[k], NBR_OWNS ? iv[u][k] : io[k],
                                        NBR_OWNS ? dv[u][k] : Do[k], at.a.slope);
                    }
                }
            }
        });
    }
}

template <int NS, bool WIDE, bool NBR_OWNS, class... Drop>
__device__ __forceinline__ void tiled_atth_grad_decode(uint32_t m, int base, int n, float (&acc)[WIDE ? 1 : NS],
                                                       const float (&a)[NS ? NS : 1], const TiledAttHLane<(NS ? NS : 1), WIDE> &ln,
                                                       const float *__restrict__ Arow, int *list, int &cnt, const float *__restrict__ B,
                                                       int N, int l, const TiledAttH &at, int self, Drop... drop) {
    while (m) {
        const int b = __builtin_clz(m);
        m &= ~(0x80000000u >> b);
        const int v = base + b;
        if (v < n && tiled_drop_kept(v, drop...)) {
            list[cnt++] = v;
            if (cnt == TILED_F32_CAP) {
                tiled_atth_grad_rows<NS, WIDE, NBR_OWNS>(acc, a, ln, Arow, list, cnt, B, N, l, at, self);
                cnt = 0;
            }
        }
    }
}

// The row view: k_tiled_att_grad's workgroup - a wave owns 8 rows of the block and is whole on each of them - with blockIdx.y the slot
// group (narrow) or the head (wide). out is [n, H]: out[o, h] = the fold of u over o's neighbours.
template <int NS, bool WIDE, bool NBR_OWNS, class... Drop>
__global__ __launch_bounds__(256) void k_tiled_att_heads_grad(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ kquad,
                                                              const uint32_t *__restrict__ tiles, uint64_t n_tiles, int n,
                                                              const float *__restrict__ A, const float *__restrict__ B, int N,
                                                              TiledAttH at, float *__restrict__ out, Drop... drop) {
    constexpr int RPG = 8, R = NS ? NS : 1, S = WIDE ? 1 : NS;
    static_assert(WIDE || NS != 0, "the narrow mapping keeps its slots in registers");
    __shared__ int lists[4][RPG][TILED_F32_CAP];
    const int rb = blockIdx.x, tid = threadIdx.x;
    const int g = __builtin_amdgcn_readfirstlane(tid / 64), l = tid % 64;
    const int nq = step128(n);
    TiledAttHLane<R, WIDE> ln;
    ln.make(at, blockIdx.y, l);

    constexpr bool NODES = tiled_has_nodes<Drop...>();
    [[maybe_unused]] const TiledNodes nodes = tiled_nodes_of(drop...);
    [[maybe_unused]] uint32_t rword = 0;   // the row bitmap's word of this block
    if constexpr (NODES) rword = tiled_nodes_word(nodes.row, rb);

    uint64_t t0 = 0, t1 = 0;   // an adjacency without tiles may come without row_ptr
    bool walk = n_tiles != 0;
    if constexpr (NODES) walk = walk && rword != 0;
    if (walk) {
        t0 = static_cast<uint64_t>(row_ptr[rb]);
        t1 = static_cast<uint64_t>(row_ptr[rb + 1]);
        t1 = t1 < n_tiles ? t1 : n_tiles;
    }
    const int row0 = rb * 32 + g * RPG;
    float acc[RPG][S], own[RPG][R];
    int cnt[RPG];
    tiled_static_for<RPG>([&](auto ri) {
        cnt[ri] = 0;
        const int row = row0 + ri < n ? row0 + ri : n - 1;   // a row past n walks zero words and stores nothing
#pragma unroll
        for (int k = 0; k < S; ++k) acc[ri][k] = 0.0f;
#pragma unroll
        for (int k = 0; k < R; ++k) own[ri][k] = NS != 0 && ln.col[k] >= 0 ? A[static_cast<uint64_t>(row) * N + ln.col[k]] : 0.0f;
    });
    const uint32_t *mine = tiles + (g * RPG + (l < RPG ? l : 0)) * 4;   // lane l < RPG: row g * RPG + l of every tile
    bool loads = l < RPG;
    if constexpr (NODES) loads = loads && tiled_nodes_bit(rword, (g * RPG + l) & 31);
    uint4 a = make_uint4(0, 0, 0, 0);
    [[maybe_unused]] uint4 nb = make_uint4(0, 0, 0, 0), nbn = make_uint4(0, 0, 0, 0);   // the neighbour bitmap's words of k-quad q / qn
    int q = -1;
    if (t0 < t1) {
        q = kquad[t0];
        if (loads) a = *reinterpret_cast<const uint4 *>(mine + t0 * 128);
        if constexpr (NODES)
            if (static_cast<unsigned>(q) < static_cast<unsigned>(nq)) nb = tiled_nodes_quad(nodes.nbr, q);
    }
    for (uint64_t t = t0; t < t1; ++t) {
        uint4 an = make_uint4(0, 0, 0, 0);
        int qn = -1;
        if (t + 1 < t1) {
            qn = kquad[t + 1];
            if (loads) an = *reinterpret_cast<const uint4 *>(mine + (t + 1) * 128);
            if constexpr (NODES)
                if (static_cast<unsigned>(qn) < static_cast<unsigned>(nq)) nbn = tiled_nodes_quad(nodes.nbr, qn);
        }
        bool decode = static_cast<unsigned>(q) < static_cast<unsigned>(nq);
        if constexpr (NODES) decode = decode && (nb.x | nb.y | nb.z | nb.w) != 0;
        if (decode) {
            const uint32_t w[4] = {a.x, a.y, a.z, a.w};
            [[maybe_unused]] const uint32_t nw[4] = {nb.x, nb.y, nb.z, nb.w};
            tiled_static_for<RPG>([&](auto ri) {
                const int row = row0 + ri < n ? row0 + ri : n - 1;
                tiled_static_for<4>([&](auto k) {
                    uint32_t mw = tiled_f32_bcast<64>(w[k], ri);
                    if constexpr (NODES) mw &= nw[k];
                    tiled_atth_grad_decode<NS, WIDE, NBR_OWNS>(mw, q * 128 + k * 32, n, acc[ri], own[ri], ln,
                                                               A + static_cast<uint64_t>(row) * N, lists[g][ri], cnt[ri], B, N, l, at, row,
                                                               tiled_drop_for(row, drop)...);
                });
            });
        }
        a = an;
        q = qn;
        if constexpr (NODES) nb = nbn;
    }
    tiled_static_for<RPG>([&](auto ri) {
        const int row = row0 + ri < n ? row0 + ri : n - 1;
        tiled_atth_grad_rows<NS, WIDE, NBR_OWNS>(acc[ri], own[ri], ln, A + static_cast<uint64_t>(row) * N, lists[g][ri], cnt[ri], B, N, l,
                                                 at, row);
        if (row0 + ri < n) {
#pragma unroll
            for (int k = 0; k < S; ++k)
                if (ln.first[k]) out[static_cast<uint64_t>(row) * at.H + ln.hd[k]] = acc[ri][k];
        }
    });
}

// ---- the row dot: out[o, h] = DOT over head h's columns of A[o] and B[o] -------------------------------------------------------------------
// a wave per (row, slot) - narrow: the 64 / P heads of the slot, each in its group of lanes - or per (row, head) - wide
template <bool WIDE>
__global__ __launch_bounds__(256) void k_rowdot_heads_f32(const float *__restrict__ A, const float *__restrict__ B, int n, int N,
                                                          TiledAttH at, int per_row, float *__restrict__ out) {
    const uint64_t unit = static_cast<uint64_t>(blockIdx.x) * 4 + threadIdx.x / 64;
    const int l = threadIdx.x % 64;
    if (unit >= static_cast<uint64_t>(n) * per_row) return;   // whole waves leave
    const int row = static_cast<int>(unit / per_row), y = static_cast<int>(unit % per_row);
    const float *__restrict__ a = A + static_cast<uint64_t>(row) * N, *__restrict__ b = B + static_cast<uint64_t>(row) * N;
    if constexpr (WIDE) {
        float t = 0.0f;
        for (int c = l; c < at.d; c += 64) t = tiled_f32_mul_add(t, a[y * at.d + c], b[y * at.d + c]);
        t = tiled_att_wave_sum(t);
        if (l == 0) out[static_cast<uint64_t>(row) * at.H + y] = t;
    } else {
        TiledAttHLane<1, false> ln;
        ln.make(at, y, l);
        const bool in = ln.col[0] >= 0;
        const float t = tiled_atth_group_sum(tiled_f32_mul_add(0.0f, in ? a[ln.col[0]] : 0.0f, in ? b[ln.col[0]] : 0.0f), at.lg);
        if (ln.first[0]) out[static_cast<uint64_t>(row) * at.H + ln.hd[0]] = t;
    }
}

// ---- the shapes (tests/tiled_attn_heads_model.py states the same choice) ---------------------------------------------------------------
// how the heads of the score gradient and of the row dot lie on a wave
struct TiledAttHShape {
    bool wide;   // d > 64
    int lg;      // narrow: log2(P), P = next_pow2(d)
    int slots;   // narrow: the slots all heads take, ceil(H * P / 64)
    int ns;      // the register slots of a workgroup: narrow 1 (a workgroup is the single-head kernel's at N = P with 64 / P heads a
                 // wave; more slots a workgroup measured slower: the neighbours' prefetch then holds 250 VGPRs); wide 4 up to d = 256,
                 // 0 = read again beyond
    int ny;      // blockIdx.y: narrow the slots, wide the heads
};
inline TiledAttHShape tiled_atth_shape(int H, int d) {
    TiledAttHShape sh{d > 64, 0, 0, 0, 0};
    if (sh.wide) {
        sh.lg = 6;
        sh.ns = d <= 256 ? 4 : 0;
        sh.ny = H;
        return sh;
    }
    while ((1 << sh.lg) < d) ++sh.lg;
    sh.slots = static_cast<int>(((static_cast<int64_t>(H) << sh.lg) + 63) / 64);
    sh.ns = 1;
    sh.ny = sh.slots;
    return sh;
}

// ---- the argument checks: the single-head entry's refusals in its order, then the heads' ---------------------------------------------------
inline bool tiled_atth_heads_bad(int heads, int N) { return heads < 1 || (N >= 1 && N % heads != 0); }

inline int tiled_atth_f32_args_ok(bool index_ok, const uint32_t *tiles, int64_t n_tiles, int n, const float *X, size_t x_elems, int N,
                                  const float *att_own, const float *att_nbr, float negative_slope, int backward, const float *shift,
                                  const float *m, const float *inv, const float *out, size_t out_elems, int heads) {
    const int rc = tiled_att_f32_args_ok(index_ok, tiles, n_tiles, n, X, x_elems, N, att_own, att_nbr, negative_slope, backward, shift, m, inv,
                                         out, out_elems);
    return tiled_atth_heads_bad(heads, N) ? QGTC_EINVAL : rc;
}
inline int tiled_atth_grad_args_ok(bool index_ok, const uint32_t *tiles, int64_t n_tiles, int n, const float *A, const float *B,
                                   size_t ab_elems, int N, const float *att_own, const float *att_nbr, float negative_slope, int nbr_owns,
                                   const float *m, const float *inv, const float *D, const float *out, size_t out_elems, int heads) {
    if (nbr_owns < 0 || nbr_owns > 1 || tiled_atth_heads_bad(heads, N) || heads > 65535) return QGTC_EINVAL;
    const float *const vec[] = {B, att_own, att_nbr, m, inv, D};
    return tiled_att_args_ok(index_ok, tiles, n_tiles, n, A, ab_elems, N, out, out_elems, static_cast<size_t>(heads), negative_slope, vec);
}

// whether a lane's CPL adjacent columns always share one head and are one aligned vector of a row (the kernels' ONE)
inline bool tiled_atth_one_head(const TiledAttH &at, const float *X, int N, int cpl) {
    return at.d % cpl == 0 && N % cpl == 0 && reinterpret_cast<uintptr_t>(X) % (sizeof(float) * cpl) == 0;
}

// ---- the launchers on the row view ----------------------------------------------------------------------------------------------------------
template <bool BWD, class... Drop>
int tiled_atth_f32_launch(const TiledRowIndex &ix, const uint32_t *tiles, int64_t n_tiles, int n, const float *X, int N,
                          const TiledAttH &at, float *m, float *inv, float *out, hipStream_t st, Drop... drop) {
    // 16 lanes a row and at most 64 columns a workgroup, whatever N: the wider row groups of the single-head table (32 and 64 lanes on
    // 4 and 8 rows each) hold a den beside every sum and measured slower than the chunks they would save
    tiled_col_width_switch(N, [&](auto cpl) {
        constexpr int LPR = 16, CPL = decltype(cpl)::value;
        const dim3 grid = tiled_row_grid(n, N, LPR * CPL);
        const uint64_t nt = static_cast<uint64_t>(n_tiles);
        if constexpr (CPL > 1) {
            if (tiled_atth_one_head(at, X, N, CPL)) {
                hipLaunchKernelGGL((k_tiled_att_heads_f32<LPR, CPL, BWD, true, Drop...>), grid, dim3(256), 0, st, ix.row_ptr, ix.kquad, tiles, nt,
                                   n, X, N, at, m, inv, out, drop...);
                return;
            }
        }
        hipLaunchKernelGGL((k_tiled_att_heads_f32<LPR, CPL, BWD, false, Drop...>), grid, dim3(256), 0, st, ix.row_ptr, ix.kquad, tiles, nt, n,
                           X, N, at, m, inv, out, drop...);
    });
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

template <class F>
void tiled_atth_grad_switch(const TiledAttHShape &sh, F &&launch) {
    if (!sh.wide) launch(tiled_int<1>{}, std::false_type{});
    else if (sh.ns) launch(tiled_int<4>{}, std::true_type{});
    else launch(tiled_int<0>{}, std::true_type{});
}

template <bool NBR_OWNS, class... Drop>
int tiled_atth_grad_launch(const TiledRowIndex &ix, const uint32_t *tiles, int64_t n_tiles, int n, const float *A, const float *B, int N,
                           const TiledAttH &at, const TiledAttHShape &sh, float *out, hipStream_t st, Drop... drop) {
    const dim3 block(256), grid((n + 31) / 32, sh.ny);
    tiled_atth_grad_switch(sh, [&](auto ns, auto wide) {
        hipLaunchKernelGGL((k_tiled_att_heads_grad<decltype(ns)::value, decltype(wide)::value, NBR_OWNS, Drop...>), grid, block, 0, st,
                           ix.row_ptr, ix.kquad, tiles, static_cast<uint64_t>(n_tiles), n, A, B, N, at, out, drop...);
    });
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

// ---- what the entries run on either view (`Index`) after their argument checks, under the mask in the pack if there is one ---------------
template <class Index, class... Drop>
int tiled_atth_f32_run(const Index &ix, const uint32_t *tiles, int64_t n_tiles, int n, const float *X, int N, const float *att_own,
                       const float *att_nbr, float negative_slope, int backward, const float *shift, float *m, float *inv, float *out,
                       int heads, void *stream, Drop... drop) {
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const TiledAttH at{TiledAtt{att_own, att_nbr, shift, backward ? inv : nullptr, nullptr, negative_slope}, heads, N / heads, 0};
    return backward ? tiled_atth_f32_launch<true>(ix, tiles, n_tiles, n, X, N, at, nullptr, nullptr, out, st, drop...)
                    : tiled_atth_f32_launch<false>(ix, tiles, n_tiles, n, X, N, at, m, inv, out, st, drop...);
}

template <class Index, class... Drop>
int tiled_atth_grad_run(const Index &ix, const uint32_t *tiles, int64_t n_tiles, int n, const float *A, const float *B, int N,
                        const float *att_own, const float *att_nbr, float negative_slope, int nbr_owns, const float *m, const float *inv,
                        const float *D, float *out, int heads, void *stream, Drop... drop) {
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const TiledAttHShape sh = tiled_atth_shape(heads, N / heads);
    if (sh.ny > 65535) return QGTC_EINVAL;
    const TiledAttH at{TiledAtt{att_own, att_nbr, m, inv, D, negative_slope}, heads, N / heads, sh.lg};
    return nbr_owns ? tiled_atth_grad_launch<true>(ix, tiles, n_tiles, n, A, B, N, at, sh, out, st, drop...)
                    : tiled_atth_grad_launch<false>(ix, tiles, n_tiles, n, A, B, N, at, sh, out, st, drop...);
}

}  // namespace
