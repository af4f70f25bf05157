// tiled_float_kernels.hip.h — part of libqgtc_hip.so (included by every float, extremum, attention, edge-value and SDDMM unit): the
// product of the tile-compressed 1-bit adjacency with a FLOAT32 right operand, out = A_tiled . X (include/qgtc.h, "Float tiled
// products"; DESIGN.md sections 6.14, 6.15) - the in-order row adder both directions share, the forward kernel, the argument checks
// of the entries and, for every float, extremum and attention unit, the host side of a launch: the kernel shapes by N and this family's
// launcher (the views' index structs and the graph part of a check are tiled_args.hip.h's).
//
// The bit products AND + popcount whole 128-bit tile rows because their operand is bit planes. Here the operand is floats and the
// tiles of real graphs are nearly empty (about 9 of 4096 cells), so a tile is read as a compressed neighbour list: the set bits of a
// tile row are decoded MSB first (count leading zeros = ascending column = ascending neighbour id) and the addressed rows of X are
// added. The contract fixes the order of the adds (ascending neighbour id, one IEEE single add each), so a lane keeps the running sum
// of its own column(s) in registers and adds the neighbours' values strictly in the order they were decoded; only the LOADS run ahead.
//
// Every template below ends in a pack `Src...`: empty, it is the code that existed before the source scale (same arguments, the same
// instructions); with one `const float *` (src_scale, n floats) a neighbour's value is multiplied by src_scale[neighbour] before it is
// added - one IEEE multiply, then one IEEE add, never fused. The pack may END in the edge-dropout mask
// (tiled_drop.hip.h): a neighbour the mask drops is never queued, so its row is never loaded. Or it may end in
// the node masks (tiled_nodes.hip.h): the neighbour bitmap is ANDed into the tile words before they are decoded,
// and a workgroup without a live output row walks nothing. Or it may end in the edge values (tiled_edge.hip.h; DESIGN.md section
// 6.15g): the decoder queues every neighbour's slot beside its id and the adder multiplies the neighbour's row by values[slot], as it
// would by a source scale.
#pragma once

#include "tiled_args.hip.h"
#include "tiled_drop.hip.h"
#include "tiled_nodes.hip.h"
#include "tiled_edge.hip.h"

namespace {

constexpr int TILED_F32_CAP = 32;   // decoded neighbour ids a row group queues in LDS before it adds their rows
constexpr int TILED_F32_AHEAD = 4;  // rows of X whose loads are in flight before the first of them is added

template <class... Mask>
inline __device__ const float *tiled_f32_src(const float *src_scale, const Mask &...) { return src_scale; }

// fl32(s + fl32(w * x)): two roundings. hipcc contracts a * b + c into one fma by default (and __fmul_rn is a plain `*` here), so the
// pair is written under `fp contract(off)`.
__device__ __forceinline__ float tiled_f32_mul_add(float s, float w, float x) {
#pragma clang fp contract(off)
    const float p = w * x;
    return s + p;
}

// s[cc] += X[list[j], c0 + cc * LPR] for j = 0 .. cnt-1, IN THAT ORDER. The loads of TILED_F32_AHEAD neighbours are issued together
// (past the end of the list the last entry is loaded again and not added); the adds of one column are a dependent chain by contract.
// A column past N reads nothing and keeps +0. `list` lives in LDS and every lane of the row group wrote every entry itself (the same
// value to the same address), so no lane reads a word another lane produced. With a source scale the neighbour's factor - one dword at
// the same address for all lanes of the group - is loaded together with its row, so it is in flight with them and adds no dependent
// latency; the term is then fl32(src_scale[v] * x), added with a separate add.
template <int LPR, int CPL, class... Src>
__device__ __forceinline__ void tiled_f32_add_rows(float (&s)[CPL], const int *list, int cnt, const float *__restrict__ X, int N, int c0,
                                                   Src... src) {
    // kept a loop: the optimizer unrolled it in some masked instantiations, which held 8 rounds of loads live (160 - 186 VGPRs)
#pragma nounroll
    for (int j = 0; j < cnt; j += TILED_F32_AHEAD) {
        float x[TILED_F32_AHEAD][CPL];
        [[maybe_unused]] float w[TILED_F32_AHEAD];
#pragma unroll
        for (int u = 0; u < TILED_F32_AHEAD; ++u) {
            const int v = list[j + u < cnt ? j + u : cnt - 1];
            const float *__restrict__ row = X + static_cast<uint64_t>(v) * N;
#pragma unroll
            for (int cc = 0; cc < CPL; ++cc) x[u][cc] = c0 + cc * LPR < N ? row[c0 + cc * LPR] : 0.0f;
            if constexpr (tiled_has_edge<Src...>()) w[u] = tiled_edge_value(j + u < cnt ? j + u : cnt - 1, src...);
            else if constexpr (tiled_pack_operands<Src...>() != 0) w[u] = tiled_f32_src(src...)[v];
        }
#pragma unroll
        for (int u = 0; u < TILED_F32_AHEAD; ++u)
            if (j + u < cnt) {
#pragma unroll
                for (int cc = 0; cc < CPL; ++cc) {
                    if constexpr (tiled_pack_operands<Src...>() != 0) s[cc] = tiled_f32_mul_add(s[cc], w[u], x[u][cc]);
                    else s[cc] += x[u][cc];
                }
            }
    }
}

// the set bits of `m`, MSB first, as neighbour ids base + (leading zeros), queued in `list`; ids from n up are dropped (the format keeps
// such cells zero; a foreign tile must not make the kernel read past X), and so are the ids a mask in the pack drops. A full queue is
// added at once.
template <int LPR, int CPL, class... Src>
__device__ __forceinline__ void tiled_f32_decode(uint32_t m, int base, int n, float (&s)[CPL], int *list, int &cnt,
                                                 const float *__restrict__ X, int N, int c0, Src... src) {
    [[maybe_unused]] int k = 0;   // with edge values: the set bits of the word consumed so far
    while (m) {
        const int b = __builtin_clz(m);
        m &= ~(0x80000000u >> b);
        const int v = base + b;
        if constexpr (tiled_has_edge<Src...>()) ++k;
        if (v < n && tiled_drop_kept(v, src...)) {
            if constexpr (tiled_has_edge<Src...>()) tiled_edge_queue(cnt, b, k - 1, src...);
            list[cnt++] = v;
            if (cnt == TILED_F32_CAP) {
                tiled_f32_add_rows<LPR, CPL>(s, list, cnt, X, N, c0, src...);
                cnt = 0;
            }
        }
    }
}

// ---- forward: out = A_tiled . X -------------------------------------------------------------------------------------------------------
// One workgroup (256 threads) per 32-row block and chunk of LPR * CPL output columns. A ROW GROUP of LPR lanes (16, 32 or a whole wave)
// owns RPG = 32 / (256 / LPR) output rows of the block, with lane l on the columns chunk + l + cc * LPR, cc < CPL: a neighbour's row of
// X is one coalesced read per cc. The group walks the block's tiles once, in k-quad order: lanes 0 .. RPG-1 load the 16-byte tile rows
// of the group's rows (the next tile's while this one is decoded), every row's 4 words are broadcast and decoded into that row's own
// queue, and a full queue is added to the row's running sums s[row][cc]; what is left is added after the walk. A row's adds are
// thereby in tile order = ascending neighbour id. Narrow outputs take narrow groups, so that a wave keeps the loads of up to 4 rows
// in flight at once. With LPR = 64 the tile words are wave-uniform (v_readlane) and the decode loop is scalar.
// The rows are stored once; SCALED multiplies by row_scale[row] first (one IEEE single multiply).
// With node masks in the pack: the workgroup reads word rb of the row bitmap (its 32 rows); when that is zero it takes an empty tile
// range without reading row_ptr, so it only stores its +0 rows; a masked-out row of a live block does not load its tile rows (zero
// words decode to nothing). The four neighbour-bitmap words of a tile's k-quad are loaded with the tile's kquad entry, one tile ahead,
// and ANDed into the broadcast words; a tile whose four bitmap words are zero is not decoded at all.
template <int LPR>
__device__ __forceinline__ uint32_t tiled_f32_bcast(uint32_t v, int src) {
    if constexpr (LPR == 64) return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), src));
    else return static_cast<uint32_t>(__shfl(static_cast<int>(v), src, LPR));
}

template <int LPR, int CPL, bool SCALED, class... Src>
__global__ __launch_bounds__(256) void k_tiled_mm_f32(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ kquad,
                                                      const uint32_t *__restrict__ tiles, uint64_t n_tiles, int n,
                                                      const float *__restrict__ X, int N, const float *__restrict__ row_scale,
                                                      float *__restrict__ out, Src... src) {
    constexpr int G = 256 / LPR, RPG = 32 / G;   // row groups per workgroup, rows per group
    constexpr bool NODES = tiled_has_nodes<Src...>();
    [[maybe_unused]] TiledNodesWalk<NODES> nd;   // the node masks' state: empty without them
    __shared__ int lists[G][RPG][TILED_F32_CAP];
    constexpr bool EDGE = tiled_has_edge<Src...>();
    [[maybe_unused]] int *slots = nullptr;   // with edge values: the slots of this row group's queued neighbours, [RPG][TILED_F32_CAP]
    if constexpr (EDGE) {
        __shared__ int edge_slots[G][RPG][TILED_F32_CAP];
        slots = &edge_slots[threadIdx.x / LPR][0][0];
    }
    [[maybe_unused]] const TiledEdge ed = tiled_edge_of(src...);
    [[maybe_unused]] int vp = 0, vr = 0;   // val_ptr of the tile being decoded; lane l < RPG: val_row of its row of that tile
    const int rb = blockIdx.x, tid = threadIdx.x;
    const int g = LPR == 64 ? __builtin_amdgcn_readfirstlane(tid / LPR) : tid / LPR;
    const int l = tid % LPR, c0 = blockIdx.y * (LPR * CPL) + l;
    const int nq = step128(n);
    if constexpr (NODES) nd.start(tiled_nodes_of(src...), rb, g * RPG + l);

    uint64_t t0 = 0, t1 = 0;   // an adjacency without tiles may come without row_ptr
    if (tiled_nodes_and<NODES>(n_tiles != 0, nd.block_live())) {
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
        if (tiled_nodes_and<NODES>(l < RPG, nd.row_live())) a = *reinterpret_cast<const uint4 *>(mine + t0 * 128);
        if constexpr (NODES) nd.load(nd.nb, q, nq);
        if constexpr (EDGE) {
            vp = static_cast<int>(ed.val_ptr[t0]);
            if (l < RPG) vr = ed.val_row[t0 * 32 + g * RPG + l];
        }
    }
    for (uint64_t t = t0; t < t1; ++t) {
        uint4 an = make_uint4(0, 0, 0, 0);
        int qn = -1;
        [[maybe_unused]] int vpn = 0, vrn = 0;
        if (t + 1 < t1) {
            qn = kquad[t + 1];
            if (tiled_nodes_and<NODES>(l < RPG, nd.row_live())) an = *reinterpret_cast<const uint4 *>(mine + (t + 1) * 128);
            if constexpr (NODES) nd.load(nd.nbn, qn, nq);
            if constexpr (EDGE) {
                vpn = static_cast<int>(ed.val_ptr[t + 1]);
                if (l < RPG) vrn = ed.val_row[(t + 1) * 32 + g * RPG + l];
            }
        }
        if (tiled_nodes_and<NODES>(static_cast<unsigned>(q) < static_cast<unsigned>(nq), nd.tile_live())) {
            const uint32_t w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
            for (int ri = 0; ri < RPG; ++ri) {
                if constexpr (EDGE) {
                    int sb = vp + static_cast<int>(tiled_f32_bcast<LPR>(static_cast<uint32_t>(vr), ri));   // the slot of the row's next set bit
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const uint32_t wk = tiled_f32_bcast<LPR>(w[k], ri);
                        tiled_f32_decode<LPR, CPL>(wk, q * 128 + k * 32, n, s[ri], lists[g][ri], cnt[ri], X, N, c0,
                                                   tiled_edge_for(TiledEdgeAtRow{slots + ri * TILED_F32_CAP, sb}, src)...);
                        sb += __builtin_popcount(wk);
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        tiled_f32_decode<LPR, CPL>(tiled_f32_bcast<LPR>(w[k], ri) & nd.word(k), q * 128 + k * 32, n, s[ri], lists[g][ri], cnt[ri], X, N,
                                                   c0, tiled_drop_for(rb * 32 + g * RPG + ri, src)...);
                }
            }
        }
        a = an;
        q = qn;
        if constexpr (NODES) nd.nb = nd.nbn;
        if constexpr (EDGE) {
            vp = vpn;
            vr = vrn;
        }
    }
#pragma unroll
    for (int ri = 0; ri < RPG; ++ri) {
        if constexpr (EDGE) tiled_f32_add_rows<LPR, CPL>(s[ri], lists[g][ri], cnt[ri], X, N, c0, tiled_edge_for(TiledEdgeAtFlush{slots + ri * TILED_F32_CAP}, src)...);
        else tiled_f32_add_rows<LPR, CPL>(s[ri], lists[g][ri], cnt[ri], X, N, c0, src...);
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

// ---- the argument checks of qgtc_tiledmm_f32 / _t and qgtc_tiledmm_f32_src / _t_src, made before any device work -----------------------------------------
inline bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// `index_ok`: every index array of the direction is there (they and `tiles` may be NULL only when n_tiles is 0)
inline int tiled_f32_args_ok(bool index_ok, const uint32_t *tiles, int64_t n_tiles, int n, const float *X, size_t x_elems, int N,
                             const float *row_scale, const float *out, size_t out_elems, const float *src_scale = nullptr) {
    if (!X || !out || N < 1 || tiled_adj_malformed(index_ok, tiles, n_tiles, n)) return QGTC_EINVAL;
    if (tiled_adj_misaligned(tiles) || !aligned4(X) || !aligned4(out) || !aligned4(row_scale) || !aligned4(src_scale))
        return QGTC_EALIGN;
    const size_t need = static_cast<size_t>(n) * static_cast<size_t>(N);
    if (x_elems < need || out_elems < need) return QGTC_ESIZE;
    return QGTC_OK;
}

// ---- the host side every float, extremum and attention unit shares: the kernel shapes by N of the two views ----------------------------
// Each kernel family has ONE launcher, at the foot of the family's header; it ends in the kernel's own trailing pack and forwards it, so
// a masked launch takes the shape its plain parent takes. The launchers of the two views are overloads on
// TiledRowIndex / TiledColIndex (tiled_args.hip.h), and the templates above them are written once for both views.
//
// The row view: lanes per output row (LPR) and columns per lane (CPL) by N, for the float sum, the extremum / select and the attention
// sum alike; launch(LPR, CPL) gets them as integral constants and makes one workgroup per 32-row block and LPR * CPL output columns
// (tiled_row_grid). tests/tiled_float_model.py FLOAT_FORWARD_VARIANTS, tiled_max_model.py MAX_FORWARD_VARIANTS and tiled_attn_model.py
// ATT_FORWARD_VARIANTS state the same choice.
template <class F>
void tiled_row_width_switch(int N, F &&launch) {
    const int width = N <= 16 ? 16 : (N <= 32 ? 32 : (N <= 64 ? 64 : (N <= 128 ? 128 : 256)));   // output columns per workgroup
    switch (width) {
        case 16: launch(tiled_int<16>{}, tiled_int<1>{}); break;
        case 32: launch(tiled_int<16>{}, tiled_int<2>{}); break;
        case 64: launch(tiled_int<16>{}, tiled_int<4>{}); break;
        case 128: launch(tiled_int<32>{}, tiled_int<4>{}); break;
        default: launch(tiled_int<64>{}, tiled_int<4>{}); break;
    }
}
inline dim3 tiled_row_grid(int n, int N, int width) { return dim3((n + 31) / 32, (N + width - 1) / width); }

// The column view: 16 lanes per output row and CPL columns per lane by N, one workgroup per k-quad and 16 * CPL output columns
// (tiled_col_grid); past WIDEST columns the output is cut into chunks of WIDEST. The float sum, the select and the attention sum go to
// 64; the extremum keeps two words of state a column and stops at 32. tests/tiled_float_model.py FLOAT_TRANSPOSED_VARIANTS,
// tiled_max_model.py MAX_TRANSPOSED_VARIANTS / SELECT_TRANSPOSED_VARIANTS and tiled_attn_model.py ATT_TRANSPOSED_VARIANTS state the same.
template <int WIDEST = 64, class F>
void tiled_col_width_switch(int N, F &&launch) {
    static_assert(WIDEST == 32 || WIDEST == 64, "16 lanes a row, 2 or 4 columns a lane at the most");
    const int width = N <= 16 ? 16 : (N <= 32 ? 32 : WIDEST);
    switch (width) {
        case 16: launch(tiled_int<1>{}); break;
        case 32: launch(tiled_int<2>{}); break;
        default:
            if constexpr (WIDEST == 64) launch(tiled_int<4>{});
            break;
    }
}
inline dim3 tiled_col_grid(int n, int N, int width) { return dim3(step128(n), (N + width - 1) / width); }

// ---- the launcher of k_tiled_mm_f32 and what the entries of the float sum share -------------------------------------------------------
template <bool SCALED, class... Pack>
int tiled_mm_f32_launch(const TiledRowIndex &ix, const uint32_t *tiles, int64_t n_tiles, int n, const float *X, int N,
                        const float *row_scale, float *out, hipStream_t st, Pack... pack) {
    tiled_row_width_switch(N, [&](auto lpr, auto cpl) {
        constexpr int LPR = decltype(lpr)::value, CPL = decltype(cpl)::value;
        hipLaunchKernelGGL((k_tiled_mm_f32<LPR, CPL, SCALED, Pack...>), tiled_row_grid(n, N, LPR * CPL), dim3(256), 0, st, ix.row_ptr,
                           ix.kquad, tiles, static_cast<uint64_t>(n_tiles), n, X, N, row_scale, out, pack...);
    });
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

// either view (`Index`), after the argument checks: SCALED by row_scale, the pack - nothing, (src_scale), (mask) or (src_scale, mask) -
// as the caller made it. An entry instantiates the kernels of the packs it passes and no others.
template <class Index, class... Pack>
int tiled_mm_f32_run(const Index &ix, const uint32_t *tiles, int64_t n_tiles, int n, const float *X, int N, const float *row_scale,
                     float *out, void *stream, Pack... pack) {
    const hipStream_t st = static_cast<hipStream_t>(stream);
    return row_scale ? tiled_mm_f32_launch<true>(ix, tiles, n_tiles, n, X, N, row_scale, out, st, pack...)
                     : tiled_mm_f32_launch<false>(ix, tiles, n_tiles, n, X, N, nullptr, out, st, pack...);
}
// under a mask the source scale is optional: it joins the pack when it is there
template <class Index, class Mask>
int tiled_mm_f32_masked(const Index &ix, const uint32_t *tiles, int64_t n_tiles, int n, const float *X, int N, const float *row_scale,
                        const float *src_scale, float *out, void *stream, const Mask &mask) {
    return src_scale ? tiled_mm_f32_run(ix, tiles, n_tiles, n, X, N, row_scale, out, stream, src_scale, mask)
                     : tiled_mm_f32_run(ix, tiles, n_tiles, n, X, N, row_scale, out, stream, mask);
}

}  // namespace
