// tiled_attn_kernels.hip.h — part of libqgtc_hip.so (included by qgtc_tiled_attn.hip and qgtc_tiled_attn_t.hip, after
// tiled_float_kernels.hip.h and tiled_max_kernels.hip.h): the softmax-weighted sum over a row's neighbours on the tile-compressed 1-bit
// adjacency, as in GAT, and its three gradients (include/qgtc.h, "Attention tiled products") - the fixed
// float32 exponential, the weight of an edge, the in-order adders, the kernels on the row view, the row dot, the argument checks
// and the launchers.
//
// The walk is the float product's (tiled_float_kernels.hip.h): a tile is read as a compressed neighbour list, decoded MSB first =
// ascending neighbour id, the ids are queued in LDS and the addressed rows are loaded TILED_F32_AHEAD at a time. The weight of edge
// (out node o, neighbour k) is not stored anywhere: it is rebuilt from two per-node scores as the rows are added,
//     e = fl(own[o] + nbr[k]),  w = EXP(fl(L(e) - shift)),  L(e) = e > 0 ? e : fl(slope * e),
// where the softmax belongs to the out node in the forward (shift = m[o], the weights also add up to den) and to the NEIGHBOUR in the
// backward (shift = m[k], w is then multiplied by inv[k]). Every lane of a row group computes the same w from the same words, so no
// lane reads what another produced. No operation is fused: every function below is under `fp contract(off)`.
#pragma once

namespace {

// the scores and the per-node softmax statistics of one launch (all float32 [n], in the adjacency's numbering)
struct TiledAtt {
    const float *__restrict__ own;     // the out node's score
    const float *__restrict__ nbr;     // the neighbour's score
    const float *__restrict__ shift;   // forward: M[o], the maximum of nbr over o's neighbours; otherwise m of the softmax's owner
    const float *__restrict__ inv;     // 1 / den of the softmax's owner (not read by the forward)
    const float *__restrict__ D;       // the score gradient only: DOT(dY[o], Y[o]) of the softmax's owner
    float slope;
};

__device__ __forceinline__ float tiled_att_lrelu(float e, float slope) {
#pragma clang fp contract(off)
    const float neg = slope * e;
    return e > 0.0f ? e : neg;
}

// EXP of include/qgtc.h for z <= 0: 0 below -87, otherwise the Cephes expf reduction and polynomial, every operation rounded on its own,
// and the power of two put into the exponent field (the result is a normal number in [FLT_MIN, 1], so that is ldexp exactly). A NaN or
// a positive z gives some value and touches no memory.
__device__ __forceinline__ float tiled_att_exp(float z) {
#pragma clang fp contract(off)
    const float kf = __builtin_rintf(z * 1.44269504088896341f);
    float r = z - kf * 0.693359375f;
    r = r - kf * -2.12194440e-4f;
    float y = 1.9875691500e-4f;
    y = y * r + 1.3981999507e-3f;
    y = y * r + 8.3334519073e-3f;
    y = y * r + 4.1665795894e-2f;
    y = y * r + 1.6666665459e-1f;
    y = y * r + 5.0000001201e-1f;
    y = y * (r * r) + r;
    y = y + 1.0f;
    const int k = static_cast<int>(kf > -127.0f ? kf : -127.0f);
    const float w = __int_as_float(__float_as_int(y) + (k << 23));
    return z < -87.0f ? 0.0f : w;
}

__device__ __forceinline__ float tiled_att_sub(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}

__device__ __forceinline__ float tiled_att_mul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}

// w of the edge whose scores add up to e = fl(po + qv), under the softmax with shift m; BWD: times that softmax's inv
template <bool BWD>
__device__ __forceinline__ float tiled_att_weight(float po, float qv, float m, float inv, float slope) {
#pragma clang fp contract(off)
    const float e = po + qv;
    const float w = tiled_att_exp(tiled_att_sub(tiled_att_lrelu(e, slope), m));
    return BWD ? tiled_att_mul(w, inv) : w;
}

// s[cc] = fl(s[cc] + fl(w_j * X[list[j], c0 + cc * LPR])) for j = 0 .. cnt-1 IN THAT ORDER, tiled_f32_add_rows with the weight rebuilt
// per neighbour: its score (backward: and its m and inv) are single dwords at one address for the whole group, loaded together with
// its row. Forward: den = fl(den + w_j) in the same order.
template <int LPR, int CPL, bool BWD>
__device__ __forceinline__ void tiled_att_add_rows(float (&s)[CPL], float &den, const int *list, int cnt, const float *__restrict__ X, int N,
                                                   int c0, const TiledAtt &att, float po, float mo) {
    for (int j = 0; j < cnt; j += TILED_F32_AHEAD) {
        float x[TILED_F32_AHEAD][CPL], qv[TILED_F32_AHEAD];
        [[maybe_unused]] float mv[TILED_F32_AHEAD], iv[TILED_F32_AHEAD];
        tiled_static_for<TILED_F32_AHEAD>([&](auto u) {
            const int v = list[j + u < cnt ? j + u : cnt - 1];
            const float *__restrict__ row = X + static_cast<uint64_t>(v) * N;
#pragma unroll
            for (int cc = 0; cc < CPL; ++cc) x[u][cc] = c0 + cc * LPR < N ? row[c0 + cc * LPR] : 0.0f;
            qv[u] = att.nbr[v];
            if constexpr (BWD) {
                mv[u] = att.shift[v];
                iv[u] = att.inv[v];
            }
        });
        tiled_static_for<TILED_F32_AHEAD>([&](auto u) {
            if (j + u < cnt) {
                float w;
                if constexpr (BWD) w = tiled_att_weight<true>(po, qv[u], mv[u], iv[u], att.slope);
                else {
                    w = tiled_att_weight<false>(po, qv[u], mo, 0.0f, att.slope);
                    den += w;
                }
#pragma unroll
                for (int cc = 0; cc < CPL; ++cc) s[cc] = tiled_f32_mul_add(s[cc], w, x[u][cc]);
            }
        });
    }
}

// (the trailing pack of every decoder and kernel below is empty, and they are the ones that existed, or holds the edge-dropout mask of
// tiled_drop.hip.h: a neighbour it drops is never queued; or the node masks of tiled_nodes.hip.h, which act as in k_tiled_mm_f32: a
// block without a live row takes an empty tile range and stores what rows without neighbours hold, a masked-out row loads no tile
// rows, and the neighbour bitmap's words of the tile's k-quad are ANDed into the decode words)
template <int LPR, int CPL, bool BWD, class... Drop>
__device__ __forceinline__ void tiled_att_decode(uint32_t m, int base, int n, float (&s)[CPL], float &den, int *list, int &cnt,
                                                 const float *__restrict__ X, int N, int c0, const TiledAtt &att, float po, float mo,
                                                 Drop... drop) {
    while (m) {
        const int b = __builtin_clz(m);
        m &= ~(0x80000000u >> b);
        const int v = base + b;
        if (v < n && tiled_drop_kept(v, drop...)) {
            list[cnt++] = v;
            if (cnt == TILED_F32_CAP) {
                tiled_att_add_rows<LPR, CPL, BWD>(s, den, list, cnt, X, N, c0, att, po, mo);
                cnt = 0;
            }
        }
    }
}

// m[o] = L(fl(own[o] + M[o])): the largest logit of o's softmax, exactly (L and the rounded add are monotone)
__device__ __forceinline__ float tiled_att_shift(float po, float M, float slope) {
#pragma clang fp contract(off)
    return tiled_att_lrelu(po + M, slope);
}

// ---- the row view ---------------------------------------------------------------------------------------------------------------------
// k_tiled_mm_f32's workgroup: one per 32-row block and chunk of LPR * CPL output columns, a row group of LPR lanes on RPG rows, the
// block's tiles walked once in k-quad order with the next tile's words loaded while this one is decoded.
//   forward (BWD false)  out[o] = fl(s * inv[o]) with inv[o] = fl(1 / den), 0 for a row without neighbours; the first column chunk
//                        also stores m[o] and inv[o];
//   backward (BWD true)  out[k] = s, the weights normalised per term by the neighbour's own statistics.
template <int LPR, int CPL, bool BWD, class... Drop>
__global__ __launch_bounds__(256) void k_tiled_att_f32(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ kquad,
                                                       const uint32_t *__restrict__ tiles, uint64_t n_tiles, int n,
                                                       const float *__restrict__ X, int N, TiledAtt att, float *__restrict__ m_out,
                                                       float *__restrict__ inv_out, float *__restrict__ out, Drop... drop) {
    constexpr int G = 256 / LPR, RPG = 32 / G;
    __shared__ int lists[G][RPG][TILED_F32_CAP];
    const int rb = blockIdx.x, tid = threadIdx.x;
    const int g = LPR == 64 ? __builtin_amdgcn_readfirstlane(tid / LPR) : tid / LPR;
    const int l = tid % LPR, c0 = blockIdx.y * (LPR * CPL) + l;
    const int nq = step128(n);

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
    float s[RPG][CPL], den[RPG], po[RPG], mo[RPG];
    int cnt[RPG];
    tiled_static_for<RPG>([&](auto ri) {
        cnt[ri] = 0;
        den[ri] = 0.0f;
        const int row = row0 + ri;
        po[ri] = row < n ? att.own[row] : 0.0f;
        mo[ri] = 0.0f;
        if constexpr (!BWD) mo[ri] = tiled_att_shift(po[ri], row < n ? att.shift[row] : 0.0f, att.slope);
#pragma unroll
        for (int cc = 0; cc < CPL; ++cc) s[ri][cc] = 0.0f;
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
                tiled_static_for<4>([&](auto k) {
                    uint32_t mw = tiled_f32_bcast<LPR>(w[k], ri);
                    if constexpr (NODES) mw &= nw[k];
                    tiled_att_decode<LPR, CPL, BWD>(mw, q * 128 + k * 32, n, s[ri], den[ri], lists[g][ri], cnt[ri], X, N, c0, att, po[ri],
                                                    mo[ri], tiled_drop_for(row0 + ri, drop)...);
                });
            });
        }
        a = an;
        q = qn;
        if constexpr (NODES) nb = nbn;
    }
    tiled_static_for<RPG>([&](auto ri) {
        tiled_att_add_rows<LPR, CPL, BWD>(s[ri], den[ri], lists[g][ri], cnt[ri], X, N, c0, att, po[ri], mo[ri]);
        const int row = row0 + ri;
        if (row < n) {
            float inv = 1.0f;
            if constexpr (!BWD) {
                inv = den[ri] > 0.0f ? __fdiv_rn(1.0f, den[ri]) : 0.0f;
                if (blockIdx.y == 0 && l == 0) {
                    m_out[row] = mo[ri];
                    inv_out[row] = inv;
                }
            }
#pragma unroll
            for (int cc = 0; cc < CPL; ++cc) {
                const int c = c0 + cc * LPR;
                if (c < N) out[static_cast<uint64_t>(row) * N + c] = BWD ? s[ri][cc] : tiled_att_mul(s[ri][cc], inv);
            }
        }
    });
}

// ---- the score gradient ---------------------------------------------------------------------------------------------------------------
// DOT of include/qgtc.h on one wave: lane j holds t_j, the in-order sum of the products of the columns j, j + 64, ...; the six
// exchange steps leave the same word in every lane (the add is commutative).
__device__ __forceinline__ float tiled_att_wave_sum(float t) {
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) t += __shfl_xor(t, h, 64);
    return t;
}

// acc = fl(acc + u) for the neighbours list[0 .. cnt) IN THAT ORDER, u = fl(alpha * fl(DOT(A[self], B[v]) - D)), times the slope where
// the edge's e is not positive. NBR_OWNS false: the softmax is the out node's (m, inv, D are mo, io, Do: this is dp); true: the
// neighbour's (they are loaded with its row: this is dq). REG: N <= 256 and the out node's own row is in `a`; otherwise both rows are
// read again for every neighbour (any N is correct, wide ones are slow).
template <bool REG, bool NBR_OWNS>
__device__ __forceinline__ void tiled_att_grad_rows(float &acc, const float (&a)[4], const float *__restrict__ Arow, const int *list,
                                                    int cnt, const float *__restrict__ B, int N, int l, const TiledAtt &att, float po,
                                                    float mo, float io, float Do) {
    for (int j = 0; j < cnt; j += TILED_F32_AHEAD) {
        [[maybe_unused]] float b[TILED_F32_AHEAD][4];
        float qv[TILED_F32_AHEAD];
        int v[TILED_F32_AHEAD];
        [[maybe_unused]] float mv[TILED_F32_AHEAD], iv[TILED_F32_AHEAD], dv[TILED_F32_AHEAD];
        tiled_static_for<TILED_F32_AHEAD>([&](auto u) {
            v[u] = list[j + u < cnt ? j + u : cnt - 1];
            if constexpr (REG) {
                const float *__restrict__ row = B + static_cast<uint64_t>(v[u]) * N;
#pragma unroll
                for (int cc = 0; cc < 4; ++cc) b[u][cc] = l + cc * 64 < N ? row[l + cc * 64] : 0.0f;
            }
            qv[u] = att.nbr[v[u]];
            if constexpr (NBR_OWNS) {
                mv[u] = att.shift[v[u]];
                iv[u] = att.inv[v[u]];
                dv[u] = att.D[v[u]];
            }
        });
        tiled_static_for<TILED_F32_AHEAD>([&](auto u) {
            if (j + u < cnt) {
                float t = 0.0f;
                if constexpr (REG) {
#pragma unroll
                    for (int cc = 0; cc < 4; ++cc) t = tiled_f32_mul_add(t, a[cc], b[u][cc]);   // past N: + fl(0 * 0), the same bits
                } else {
                    const float *__restrict__ row = B + static_cast<uint64_t>(v[u]) * N;
                    for (int c = l; c < N; c += 64) t = tiled_f32_mul_add(t, Arow[c], row[c]);
                }
                t = tiled_att_wave_sum(t);
                const float m = NBR_OWNS ? mv[u] : mo, inv = NBR_OWNS ? iv[u] : io, D = NBR_OWNS ? dv[u] : Do;
                const float alpha = tiled_att_weight<true>(po, qv[u], m, inv, att.slope);
                float g = tiled_att_mul(alpha, tiled_att_sub(t, D));
                {
#pragma clang fp contract(off)
                    const float e = po + qv[u];
                    if (!(e > 0.0f)) g = att.slope * g;
                    acc = acc + g;
                }
            }
        });
    }
}

template <bool REG, bool NBR_OWNS, class... Drop>
__device__ __forceinline__ void tiled_att_grad_decode(uint32_t m, int base, int n, float &acc, const float (&a)[4],
                                                      const float *__restrict__ Arow, int *list, int &cnt, const float *__restrict__ B,
                                                      int N, int l, const TiledAtt &att, float po, float mo, float io, float Do,
                                                      Drop... drop) {
    while (m) {
        const int b = __builtin_clz(m);
        m &= ~(0x80000000u >> b);
        const int v = base + b;
        if (v < n && tiled_drop_kept(v, drop...)) {
            list[cnt++] = v;
            if (cnt == TILED_F32_CAP) {
                tiled_att_grad_rows<REG, NBR_OWNS>(acc, a, Arow, list, cnt, B, N, l, att, po, mo, io, Do);
                cnt = 0;
            }
        }
    }
}

// The row view: k_tiled_mm_f32's workgroup at 64 lanes a row - a wave owns 8 rows of the block and is whole on each of them, lane j on
// the columns j + 64 cc. out is float32 [n]: out[o] = the fold of u over o's neighbours. A is the matrix of the out node's rows, B the
// neighbours' (dp: dY and X; dq: X and dY - the products are commutative, so DOT is the same word).
template <bool REG, bool NBR_OWNS, class... Drop>
__global__ __launch_bounds__(256) void k_tiled_att_grad(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ kquad,
                                                        const uint32_t *__restrict__ tiles, uint64_t n_tiles, int n,
                                                        const float *__restrict__ A, const float *__restrict__ B, int N, TiledAtt att,
                                                        float *__restrict__ out, Drop... drop) {
    constexpr int RPG = 8;
    __shared__ int lists[4][RPG][TILED_F32_CAP];
    const int rb = blockIdx.x, tid = threadIdx.x;
    const int g = __builtin_amdgcn_readfirstlane(tid / 64), l = tid % 64;
    const int nq = step128(n);

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
    float acc[RPG], own[RPG][4], po[RPG], mo[RPG], io[RPG], Do[RPG];
    int cnt[RPG];
    tiled_static_for<RPG>([&](auto ri) {
        cnt[ri] = 0;
        acc[ri] = 0.0f;
        const int row = row0 + ri < n ? row0 + ri : n - 1;   // a row past n walks zero words and stores nothing
        po[ri] = att.own[row];
        mo[ri] = io[ri] = Do[ri] = 0.0f;
        if constexpr (!NBR_OWNS) {
            mo[ri] = att.shift[row];
            io[ri] = att.inv[row];
            Do[ri] = att.D[row];
        }
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) own[ri][cc] = REG && l + cc * 64 < N ? A[static_cast<uint64_t>(row) * N + l + cc * 64] : 0.0f;
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
                    tiled_att_grad_decode<REG, NBR_OWNS>(mw, q * 128 + k * 32, n, acc[ri], own[ri], A + static_cast<uint64_t>(row) * N,
                                                         lists[g][ri], cnt[ri], B, N, l, att, po[ri], mo[ri], io[ri], Do[ri],
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
        tiled_att_grad_rows<REG, NBR_OWNS>(acc[ri], own[ri], A + static_cast<uint64_t>(row) * N, lists[g][ri], cnt[ri], B, N, l, att,
                                           po[ri], mo[ri], io[ri], Do[ri]);
        if (row0 + ri < n && l == 0) out[row0 + ri] = acc[ri];
    });
}

// ---- the row dot: out[o] = DOT(A[o], B[o]), one wave a row ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rowdot_f32(const float *__restrict__ A, const float *__restrict__ B, int n, int N,
                                                    float *__restrict__ out) {
    const int row = blockIdx.x * 4 + threadIdx.x / 64, l = threadIdx.x % 64;
    if (row >= n) return;   // whole waves leave
    const float *__restrict__ a = A + static_cast<uint64_t>(row) * N, *__restrict__ b = B + static_cast<uint64_t>(row) * N;
    float t = 0.0f;
    for (int c = l; c < N; c += 64) t = tiled_f32_mul_add(t, a[c], b[c]);
    t = tiled_att_wave_sum(t);
    if (l == 0) out[row] = t;
}

// ---- the argument checks, made before any device work -------------------------------------------------------------------------------------
// tiled_f32_args_ok's refusals in its order (invalid, then alignment, then sizes) with the per-node vectors beside the matrices:
// QGTC_EINVAL also for a missing vector and a slope outside [0, 1] (a NaN included); QGTC_EALIGN also for a vector off a 4-byte boundary.
inline bool tiled_att_slope_ok(float slope) { return slope >= 0.0f && slope <= 1.0f; }

template <size_t K>
inline int tiled_att_args_ok(bool index_ok, const uint32_t *tiles, int64_t n_tiles, int n, const float *X, size_t x_elems, int N,
                             const float *out, size_t out_elems, size_t out_need_cols, float slope, const float *const (&vec)[K]) {
    if (!tiled_att_slope_ok(slope)) return QGTC_EINVAL;
    for (const float *v : vec)
        if (!v) return QGTC_EINVAL;
    if (!X || !out || N < 1 || tiled_adj_malformed(index_ok, tiles, n_tiles, n)) return QGTC_EINVAL;
    if (tiled_adj_misaligned(tiles) || !aligned4(X) || !aligned4(out)) return QGTC_EALIGN;
    for (const float *v : vec)
        if (!aligned4(v)) return QGTC_EALIGN;
    const size_t need = static_cast<size_t>(n) * static_cast<size_t>(N);
    if (x_elems < need || out_elems < static_cast<size_t>(n) * out_need_cols) return QGTC_ESIZE;
    return QGTC_OK;
}

// what qgtc_tiledatt_f32 / qgtc_tiledatt_grad_f32 and their twins on either view and under either mask check of their own arguments
inline int tiled_att_f32_args_ok(bool index_ok, const uint32_t *tiles, int64_t n_tiles, int n, const float *X, size_t x_elems, int N,
                                 const float *att_own, const float *att_nbr, float negative_slope, int backward, const float *shift,
                                 const float *m, const float *inv, const float *out, size_t out_elems) {
    if (backward < 0 || backward > 1) return QGTC_EINVAL;
    const float *const vec[] = {att_own, att_nbr, shift, inv, backward ? shift : m};
    return tiled_att_args_ok(index_ok, tiles, n_tiles, n, X, x_elems, N, out, out_elems, static_cast<size_t>(N > 0 ? N : 0), negative_slope,
                             vec);
}
inline int tiled_att_grad_args_ok(bool index_ok, const uint32_t *tiles, int64_t n_tiles, int n, const float *A, const float *B,
                                  size_t ab_elems, int N, const float *att_own, const float *att_nbr, float negative_slope, int nbr_owns,
                                  const float *m, const float *inv, const float *D, const float *out, size_t out_elems) {
    if (nbr_owns < 0 || nbr_owns > 1) return QGTC_EINVAL;
    const float *const vec[] = {B, att_own, att_nbr, m, inv, D};
    return tiled_att_args_ok(index_ok, tiles, n_tiles, n, A, ab_elems, N, out, out_elems, 1, negative_slope, vec);
}

// ---- the launchers of k_tiled_att_f32 (the shapes are the float product's: tiled_row_width_switch) and k_tiled_att_grad ------------------
template <bool BWD, class... Drop>
int tiled_att_f32_launch(const TiledRowIndex &ix, const uint32_t *tiles, int64_t n_tiles, int n, const float *X, int N, const TiledAtt &att,
                         float *m, float *inv, float *out, hipStream_t st, Drop... drop) {
    tiled_row_width_switch(N, [&](auto lpr, auto cpl) {
        constexpr int LPR = decltype(lpr)::value, CPL = decltype(cpl)::value;
        hipLaunchKernelGGL((k_tiled_att_f32<LPR, CPL, BWD, Drop...>), tiled_row_grid(n, N, LPR * CPL), dim3(256), 0, st, ix.row_ptr, ix.kquad,
                           tiles, static_cast<uint64_t>(n_tiles), n, X, N, att, m, inv, out, drop...);
    });
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

// the out node's row in registers (REG) up to N = 256, read again per neighbour beyond (tests/tiled_attn_model.py, ATT_GRAD_VARIANTS)
template <bool NBR_OWNS, class... Drop>
int tiled_att_grad_launch(const TiledRowIndex &ix, const uint32_t *tiles, int64_t n_tiles, int n, const float *A, const float *B, int N,
                          const TiledAtt &att, float *out, hipStream_t st, Drop... drop) {
    const dim3 block(256), grid((n + 31) / 32);
    const uint64_t nt = static_cast<uint64_t>(n_tiles);
    if (N <= 256)
        hipLaunchKernelGGL((k_tiled_att_grad<true, NBR_OWNS, Drop...>), grid, block, 0, st, ix.row_ptr, ix.kquad, tiles, nt, n, A, B, N, att,
                           out, drop...);
    else
        hipLaunchKernelGGL((k_tiled_att_grad<false, NBR_OWNS, Drop...>), grid, block, 0, st, ix.row_ptr, ix.kquad, tiles, nt, n, A, B, N, att,
                           out, drop...);
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

// ---- what the attention entries run on either view (`Index`) after their argument checks, under the mask in the pack if there is one ----
template <class Index, class... Drop>
int tiled_att_f32_run(const Index &ix, const uint32_t *tiles, int64_t n_tiles, int n, const float *X, int N, const float *att_own,
                      const float *att_nbr, float negative_slope, int backward, const float *shift, float *m, float *inv, float *out,
                      void *stream, Drop... drop) {
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const TiledAtt att{att_own, att_nbr, shift, backward ? inv : nullptr, nullptr, negative_slope};   // the forward only writes inv
    return backward ? tiled_att_f32_launch<true>(ix, tiles, n_tiles, n, X, N, att, nullptr, nullptr, out, st, drop...)
                    : tiled_att_f32_launch<false>(ix, tiles, n_tiles, n, X, N, att, m, inv, out, st, drop...);
}

template <class Index, class... Drop>
int tiled_att_grad_run(const Index &ix, const uint32_t *tiles, int64_t n_tiles, int n, const float *A, const float *B, int N,
                       const float *att_own, const float *att_nbr, float negative_slope, int nbr_owns, const float *m, const float *inv,
                       const float *D, float *out, void *stream, Drop... drop) {
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const TiledAtt att{att_own, att_nbr, m, inv, D, negative_slope};
    return nbr_owns ? tiled_att_grad_launch<true>(ix, tiles, n_tiles, n, A, B, N, att, out, st, drop...)
                    : tiled_att_grad_launch<false>(ix, tiles, n_tiles, n, A, B, N, att, out, st, drop...);
}

}  // namespace
