// tiled_max_kernels.hip.h — part of libqgtc_hip.so (included by qgtc_tiled_max.hip and qgtc_tiled_max_t.hip, after
// tiled_float_kernels.hip.h): the element-wise maximum / minimum over a row's neighbours on the tile-compressed 1-bit adjacency and the
// gather that is its gradient (include/qgtc.h, "Extremum tiled products") - the two reducers, the in-order fold
// both directions share, the kernel on the row view, the argument checks of the entries and the launcher.
//
// The walk is the float product's (tiled_float_kernels.hip.h): a tile is read as a compressed neighbour list, decoded MSB first =
// ascending neighbour id, the ids are queued in LDS and the addressed rows are loaded TILED_F32_AHEAD at a time. What changes is what
// a lane does with a loaded row, and that is a REDUCER: a small struct that holds the operand pointers and folds the rows of a queue,
// in queue order, into a per-column state (a running value and, for the extremum, the id of the neighbour that supplied it).
//   TiledExtremum<MIN>  s, a start as (+0, -1); neighbour v with value x replaces them when the state is empty (a < 0), or s is not a
//                       NaN and x is a NaN or x > s (MIN: x < s). So the first NaN in id order wins and stays, otherwise the lowest
//                       id among those attaining the extremum, -0 and +0 compare equal, and the value is moved, never computed.
//   TiledSelect         s starts as +0; neighbour r adds dY[r, c] when arg[r, c] is the output row's own id. dY and arg of a
//                       neighbour row are loaded together, both coalesced; arg is only ever compared.
#pragma once

#include <type_traits>
#include <utility>

namespace {

// f(integral_constant 0), ..., f(integral_constant K - 1): the loops over a row group's rows index per-row register state, so their
// bounds are unrolled by the language and not left to the optimizer (which gave up on some instantiations and spilled the state)
template <class F, int... I>
__device__ __forceinline__ void tiled_static_for(F &&f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}
template <int K, class F>
__device__ __forceinline__ void tiled_static_for(F &&f) {
    tiled_static_for(f, std::make_integer_sequence<int, K>{});
}

template <int CPL>
struct TiledRedState {
    float s[CPL];
    int a[CPL];   // the extremum's winner (-1: no neighbour yet); unused by the select
};

template <bool MIN>
struct TiledExtremum {
    static constexpr int WORDS = 2;   // 32-bit words of state a column keeps between rounds of the transposed kernel
    const float *__restrict__ X;
    float *__restrict__ out;
    int32_t *__restrict__ arg;        // may be NULL

    // the rows list[0 .. cnt) of X folded into st IN THAT ORDER; columns past N read nothing (their state is never stored)
    template <int LPR, int CPL>
    __device__ __forceinline__ void rows(TiledRedState<CPL> &st, int, const int *list, int cnt, int N, int c0) const {
        for (int j = 0; j < cnt; j += TILED_F32_AHEAD) {
            float x[TILED_F32_AHEAD][CPL];
            int v[TILED_F32_AHEAD];
            tiled_static_for<TILED_F32_AHEAD>([&](auto u) {
                v[u] = list[j + u < cnt ? j + u : cnt - 1];
                const float *__restrict__ row = X + static_cast<uint64_t>(v[u]) * N;
#pragma unroll
                for (int cc = 0; cc < CPL; ++cc) x[u][cc] = c0 + cc * LPR < N ? row[c0 + cc * LPR] : 0.0f;
            });
            tiled_static_for<TILED_F32_AHEAD>([&](auto u) {
                if (j + u < cnt) {
#pragma unroll
                    for (int cc = 0; cc < CPL; ++cc) {
                        const float s = st.s[cc], xv = x[u][cc];
                        const bool take = st.a[cc] < 0 || (s == s && (xv != xv || (MIN ? xv < s : xv > s)));
                        st.s[cc] = take ? xv : s;
                        st.a[cc] = take ? v[u] : st.a[cc];
                    }
                }
            });
        }
    }

    __device__ __forceinline__ void store(uint64_t at, float s, int a) const {
        out[at] = s;
        if (arg) arg[at] = a;
    }
};

struct TiledSelect {
    static constexpr int WORDS = 1;
    const float *__restrict__ dY;
    const int32_t *__restrict__ arg;
    float *__restrict__ out;

    // s += dY[r, c] for the rows r = list[0 .. cnt), IN THAT ORDER, where arg[r, c] == self (the output row). A column past N loads
    // arg = -1, which no output row equals.
    template <int LPR, int CPL>
    __device__ __forceinline__ void rows(TiledRedState<CPL> &st, int self, const int *list, int cnt, int N, int c0) const {
        for (int j = 0; j < cnt; j += TILED_F32_AHEAD) {
            float d[TILED_F32_AHEAD][CPL];
            int w[TILED_F32_AHEAD][CPL];
#pragma unroll
            for (int u = 0; u < TILED_F32_AHEAD; ++u) {
                const uint64_t at = static_cast<uint64_t>(list[j + u < cnt ? j + u : cnt - 1]) * N;
#pragma unroll
                for (int cc = 0; cc < CPL; ++cc) {
                    const bool in = c0 + cc * LPR < N;
                    d[u][cc] = in ? dY[at + c0 + cc * LPR] : 0.0f;
                    w[u][cc] = in ? arg[at + c0 + cc * LPR] : -1;
                }
            }
#pragma unroll
            for (int u = 0; u < TILED_F32_AHEAD; ++u)
                if (j + u < cnt) {
#pragma unroll
                    for (int cc = 0; cc < CPL; ++cc) st.s[cc] = w[u][cc] == self ? st.s[cc] + d[u][cc] : st.s[cc];
                }
        }
    }

    __device__ __forceinline__ void store(uint64_t at, float s, int) const { out[at] = s; }
};

// tiled_f32_decode with a reducer: the set bits of `m`, MSB first, as neighbour ids base + (leading zeros), queued in `list`; ids from n
// up are dropped, so nothing is read past the operands, and so are the ids the edge-dropout mask drops when the trailing pack holds one
// (tiled_drop.hip.h; empty, this is the decoder that existed). A full queue is folded at once.
template <int LPR, int CPL, class Red, class... Drop>
__device__ __forceinline__ void tiled_red_decode(uint32_t m, int base, int n, TiledRedState<CPL> &st, int self, int *list, int &cnt,
                                                 const Red &red, int N, int c0, Drop... drop) {
    while (m) {
        const int b = __builtin_clz(m);
        m &= ~(0x80000000u >> b);
        const int v = base + b;
        if (v < n && tiled_drop_kept(v, drop...)) {
            list[cnt++] = v;
            if (cnt == TILED_F32_CAP) {
                red.template rows<LPR, CPL>(st, self, list, cnt, N, c0);
                cnt = 0;
            }
        }
    }
}

// ---- the row view: out[r] = reduce over the set cells of row r ----------------------------------------------------------------------
// k_tiled_mm_f32's workgroup: one per 32-row block and chunk of LPR * CPL output columns, a row group of LPR lanes on RPG rows, the
// block's tiles walked once in k-quad order with the next tile's words loaded while this one is decoded. Node masks at the end of the
// pack (tiled_nodes.hip.h) act as they do there: a block without a live row takes an empty tile range, a masked-out row loads no tile
// rows, and the neighbour bitmap's words of the tile's k-quad are ANDed into the decode words.
template <int LPR, int CPL, class Red, class... Drop>
__global__ __launch_bounds__(256) void k_tiled_red_f32(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ kquad,
                                                       const uint32_t *__restrict__ tiles, uint64_t n_tiles, int n, int N, Red red,
                                                       Drop... drop) {
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
    TiledRedState<CPL> st[RPG];
    int cnt[RPG];
    tiled_static_for<RPG>([&](auto ri) {
        cnt[ri] = 0;
#pragma unroll
        for (int cc = 0; cc < CPL; ++cc) {
            st[ri].s[cc] = 0.0f;
            st[ri].a[cc] = -1;
        }
    });
    const int row0 = rb * 32 + g * RPG;
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
                    uint32_t m = tiled_f32_bcast<LPR>(w[k], ri);
                    if constexpr (NODES) m &= nw[k];
                    tiled_red_decode<LPR, CPL>(m, q * 128 + k * 32, n, st[ri], row0 + ri, lists[g][ri], cnt[ri], red, N, c0,
                                               tiled_drop_for(row0 + ri, drop)...);
                });
            });
        }
        a = an;
        q = qn;
        if constexpr (NODES) nb = nbn;
    }
    tiled_static_for<RPG>([&](auto ri) {
        red.template rows<LPR, CPL>(st[ri], row0 + ri, lists[g][ri], cnt[ri], N, c0);
        const int row = row0 + ri;
        if (row < n) {
#pragma unroll
            for (int cc = 0; cc < CPL; ++cc) {
                const int c = c0 + cc * LPR;
                if (c < N) red.store(static_cast<uint64_t>(row) * N + c, st[ri].s[cc], st[ri].a[cc]);
            }
        }
    });
}

// ---- the argument checks of qgtc_tiledmax_f32 / _t and qgtc_tiledsel_f32 / _t, made before any device work ---------------------------------
// tiled_f32_args_ok's refusals in its order (invalid, then alignment, then sizes) with `arg` beside `out`: QGTC_EINVAL also for an op
// outside {0, 1} or a missing arg where it is an operand; QGTC_EALIGN also for arg off a 4-byte boundary; QGTC_ESIZE also for
// arg_elems < n * N when arg is given.
inline int tiled_red_args_ok(bool index_ok, const uint32_t *tiles, int64_t n_tiles, int n, const float *X, size_t x_elems, int N,
                             const float *out, size_t out_elems, const int32_t *arg, size_t arg_elems, bool arg_required, int op) {
    if (op < 0 || op > 1 || (arg_required && !arg)) return QGTC_EINVAL;
    const int rc = tiled_f32_args_ok(index_ok, tiles, n_tiles, n, X, x_elems, N, nullptr, out, out_elems);
    if (rc == QGTC_EINVAL || rc == QGTC_EALIGN) return rc;
    if (!aligned4(arg)) return QGTC_EALIGN;
    if (rc != QGTC_OK) return rc;
    if (arg && arg_elems < static_cast<size_t>(n) * static_cast<size_t>(N)) return QGTC_ESIZE;
    return QGTC_OK;
}

// ---- the launcher of k_tiled_red_f32 (the shapes are the float product's: tiled_row_width_switch) and the extremum entries' choice --------
template <class Red, class... Drop>
int tiled_red_f32_launch(const TiledRowIndex &ix, const uint32_t *tiles, int64_t n_tiles, int n, int N, const Red &red, hipStream_t st,
                         Drop... drop) {
    tiled_row_width_switch(N, [&](auto lpr, auto cpl) {
        constexpr int LPR = decltype(lpr)::value, CPL = decltype(cpl)::value;
        hipLaunchKernelGGL((k_tiled_red_f32<LPR, CPL, Red, Drop...>), tiled_row_grid(n, N, LPR * CPL), dim3(256), 0, st, ix.row_ptr, ix.kquad,
                           tiles, static_cast<uint64_t>(n_tiles), n, N, red, drop...);
    });
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

// either view (`Index`), after the argument checks: the maximum (op 0) or the minimum (op 1), under the mask in the pack if there is one
template <class Index, class... Drop>
int tiled_extremum_run(const Index &ix, const uint32_t *tiles, int64_t n_tiles, int n, const float *X, int N, int op, float *out,
                       int32_t *arg, void *stream, Drop... drop) {
    const hipStream_t st = static_cast<hipStream_t>(stream);
    return op ? tiled_red_f32_launch(ix, tiles, n_tiles, n, N, TiledExtremum<true>{X, out, arg}, st, drop...)
              : tiled_red_f32_launch(ix, tiles, n_tiles, n, N, TiledExtremum<false>{X, out, arg}, st, drop...);
}

}  // namespace
