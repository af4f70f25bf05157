// tiled_codes_edge_kernels.hip.h — part of libqgtc_hip.so (included by qgtc_tiled_codes_edge.hip and qgtc_tiled_codes_edge_t.hip, after
// common.hip.h and bitmm_popcount.hip.h): the edge-weighted neighbour sum on byte codes (include/qgtc_codes_edge.h; DESIGN.md section
// 6.15v) - per output row o of the view and column c of head h = c / (N / heads)
//     S[o][c] = sum over the live neighbours k of values[slot(o, k) * heads + h] * (Q[k][c] - z),     y = scale * S (* row_scale[o])
// on the tile-compressed adjacency, on both views, under node masks, stored as float32 or as codes under another row.
//
// The geometry is that of tiled_codes_walk.hip.h: one workgroup of 256 per 32-row block (row view) or k-quad (column view), row groups
// of LPR lanes, a lane on four adjacent columns with one dword gathered per neighbour, ids decoded MSB first into an LDS queue of
// TILED_U8_CAP, loads TILED_U8_AHEAD ahead. The walks are written out here, not taken from there: beside every id a SLOT is queued, and
// finding it needs the tile's RAW words (a masked-out bit still owns a slot), val_ptr and val_row, which the shared walks do not carry.
// The launcher, the width rule and the argument predicates are tiled_codes_kernels.hip.h's; the slot arithmetic is tiled_edge.hip.h's.
//
// Arithmetic: a lane keeps sum w * q in four float accumulators and sum w in a fifth; the zero point leaves in the epilogue,
// S = fma(-z, sum w, sum w q). Per gathered dword that is 4 byte-to-float conversions, 4 FMAs (2 packed) and 1 add; folding (q - z) into
// every term would cost 4 more subtractions a dword. There is no add-order contract: float32, fused, packed where the compiler likes.
// The weight of a term is one dword at the same address for every lane of a head (d % 4 == 0, so a lane's four columns share a head);
// it is loaded with the code dword, so both are in flight together. The surplus slots of a load-ahead round get the weight 0.
#pragma once

#include "tiled_codes_kernels.hip.h"
#include "tiled_edge.hip.h"

namespace {

typedef float tiled_u8e_f2 __attribute__((ext_vector_type(2)));

// the edge values as one kernel argument: TiledEdge and the heads; `values` is float32 [n_values][heads]
struct TiledU8Edge {
    const int64_t *val_ptr;
    const int16_t *val_row;
    const float *values;
    int n_values, heads;
};

// the output as one kernel argument; a kernel reads the fields of its own form only
struct TiledU8EdgeOut {
    void *p;             // CODES: code matrix [n, N], rows ld bytes apart; otherwise float32 [n, N], contiguous
    size_t ld;
    const float4 *oqp;   // CODES: the output's qparams row (scale, zero point, inverse scale, 0)
    float qmax;          // CODES: 2^out_bits - 1
};

// a lane's state for one output row: sum w * q of its four columns (two packed pairs) and sum w
struct TiledU8Weighted {
    tiled_u8e_f2 lo, hi;
    float sw;
    __device__ __forceinline__ void reset() {
        lo = hi = tiled_u8e_f2{0.0f, 0.0f};
        sw = 0.0f;
    }
};

// what a lane needs of the values: those of its own head (values + h), the stride between slots, the bound
struct TiledU8EdgeLane {
    const float *vh;
    int n_values, heads;
};
__device__ __forceinline__ TiledU8EdgeLane tiled_u8e_lane(const TiledU8Edge &e, int cb, int N) {
    const int h = cb < N ? cb / (N / e.heads) : 0;   // a lane past N stores nothing
    return TiledU8EdgeLane{e.values + h, e.n_values, e.heads};
}

// r += values[slots[j]] * Q[list[j]][cb .. cb + 3], j < cnt. The code dwords and the weights of TILED_U8_AHEAD neighbours are loaded
// together; past the end the last entry is loaded again with the weight 0, and so is a slot outside [0, n_values): every slot of a
// round is then reduced alike, without a branch. `list` / `slots`: LDS, every lane wrote every entry itself.
__device__ __forceinline__ void tiled_u8e_fold(TiledU8Weighted &r, const int *list, const int *slots, int cnt, const uint8_t *__restrict__ Q,
                                               size_t ld, int cb, bool mine, const TiledU8EdgeLane &e) {
#pragma nounroll
    for (int j = 0; j < cnt; j += TILED_U8_AHEAD) {
        uint32_t w[TILED_U8_AHEAD];
        float x[TILED_U8_AHEAD];
#pragma unroll
        for (int u = 0; u < TILED_U8_AHEAD; ++u) {
            const int i = j + u < cnt ? j + u : cnt - 1;
            const int v = list[i], sl = slots[i];
            const bool ok = mine && j + u < cnt && static_cast<unsigned>(sl) < static_cast<unsigned>(e.n_values);
            w[u] = mine ? *reinterpret_cast<const uint32_t *>(Q + static_cast<size_t>(v) * ld + cb) : 0u;
            x[u] = ok ? e.vh[static_cast<size_t>(sl) * e.heads] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < TILED_U8_AHEAD; ++u) {
            const tiled_u8e_f2 xx{x[u], x[u]};
            const tiled_u8e_f2 q01{static_cast<float>(w[u] & 0xffu), static_cast<float>((w[u] >> 8) & 0xffu)};
            const tiled_u8e_f2 q23{static_cast<float>((w[u] >> 16) & 0xffu), static_cast<float>(w[u] >> 24)};
            r.lo = __builtin_elementwise_fma(xx, q01, r.lo);
            r.hi = __builtin_elementwise_fma(xx, q23, r.hi);
            r.sw += x[u];
        }
    }
}

// the set bits of `live`, MSB first, as ids base + (leading zeros), queued with their slots; ids from n up are dropped. `raw` is the
// tile word as stored, `live` its bits under the masks and `sb` the slot of raw's first set bit: the slot of bit b is sb plus the RAW
// bits above b. A full queue is reduced at once.
__device__ __forceinline__ void tiled_u8e_decode_row(uint32_t live, uint32_t raw, int sb, int base, int n, TiledU8Weighted &r, int *list,
                                                     int *slots, int &cnt, const uint8_t *__restrict__ Q, size_t ld, int cb, bool mine,
                                                     const TiledU8EdgeLane &e) {
    while (live) {
        const int b = __builtin_clz(live);
        live &= ~(0x80000000u >> b);
        const int v = base + b;
        if (v < n) {
            slots[cnt] = sb + __builtin_popcount(raw & ~(0xffffffffu >> b));
            list[cnt++] = v;
            if (cnt == TILED_U8_CAP) {
                tiled_u8e_fold(r, list, slots, cnt, Q, ld, cb, mine, e);
                cnt = 0;
            }
        }
    }
}

// the same for a column mask of a staged tile: bit b is tile row b, whose raw words are raw[b * 4 ..] and whose in-tile prefix is
// vrow[b]; `vp` the tile's val_ptr, `col` the column (0 .. 127)
__device__ __forceinline__ void tiled_u8e_decode_col(uint32_t live, const uint32_t *raw, const int *vrow, int vp, int col, int base, int n,
                                                     TiledU8Weighted &r, int *list, int *slots, int &cnt, const uint8_t *__restrict__ Q,
                                                     size_t ld, int cb, bool mine, const TiledU8EdgeLane &e) {
    while (live) {
        const int b = __builtin_clz(live);
        live &= ~(0x80000000u >> b);
        const int v = base + b;
        if (v < n) {
            const uint32_t *rw = raw + b * 4;
            slots[cnt] = vp + vrow[b] + tiled_edge_row_before(rw[0], rw[1], rw[2], rw[3], col);
            list[cnt++] = v;
            if (cnt == TILED_U8_CAP) {
                tiled_u8e_fold(r, list, slots, cnt, Q, ld, cb, mine, e);
                cnt = 0;
            }
        }
    }
}

// the epilogue of one output row's four columns: S = fma(-z, sum w, sum w q), y = S * scale (* row_scale[row]) + 0 - the last add makes
// every zero +0, so a row without a term is +0 whatever the sign of its scale - stored as float32 or through the quantiser as one dword
template <bool CODES>
__device__ __forceinline__ void tiled_u8e_store(const TiledU8Weighted &r, int row, int cb, int N, const float4 *__restrict__ qp,
                                                const float *__restrict__ row_scale, const TiledU8EdgeOut &out) {
    if (cb >= N) return;
    const float4 g = qp[0];
    const float rs = row_scale ? row_scale[row] : 1.0f;
    const float s[4] = {r.lo.x, r.lo.y, r.hi.x, r.hi.y};
    float y[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        y[k] = fmaf(-g.y, r.sw, s[k]) * g.x;
        if (row_scale) y[k] *= rs;
        y[k] += 0.0f;
    }
    if constexpr (CODES) {
        const float4 og = out.oqp[0];
        uint32_t word = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) word |= (cb + k < N ? codes_quant(y[k], og.z, og.y, out.qmax) : 0u) << (8 * k);   // bytes N .. PAD4(N) - 1: 0
        *reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(out.p) + static_cast<uint64_t>(row) * out.ld + cb) = word;
    } else {
        float *o = static_cast<float *>(out.p) + static_cast<uint64_t>(row) * N;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (cb + k < N) o[cb + k] = y[k];
    }
}

// ---- the row view ------------------------------------------------------------------------------------------------------------------------
// tiled_u8_row_walk with slots. The lanes l < RPG that load the tile rows of the group's rows also load val_row of their row; val_ptr of
// the tile is uniform. Both run one tile ahead with the words. A row's words are broadcast RAW: the neighbour bitmap is ANDed into the
// copy that is decoded, while the slot base runs over the raw popcounts.
template <int LPR, bool CODES>
__global__ __launch_bounds__(256) void k_tiled_mm_u8_edge(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ kquad,
                                                          const uint32_t *__restrict__ tiles, uint64_t n_tiles, int n,
                                                          const uint8_t *__restrict__ Q, size_t ld, int N, const float4 *__restrict__ qp,
                                                          const float *__restrict__ row_scale, TiledU8Edge ed, TiledU8EdgeOut out,
                                                          TiledNodes nodes) {
    constexpr int G = 256 / LPR, RPG = 32 / G;   // row groups per workgroup, rows per group
    __shared__ int lists[G][RPG][TILED_U8_CAP], slots[G][RPG][TILED_U8_CAP];
    const int rb = blockIdx.x, tid = threadIdx.x;
    const int g = LPR == 64 ? __builtin_amdgcn_readfirstlane(tid / LPR) : tid / LPR;
    const int l = tid % LPR, cb = blockIdx.y * (LPR * 4) + l * 4;
    const bool mine_cols = cb < N;
    const TiledU8EdgeLane e = tiled_u8e_lane(ed, cb, N);
    TiledNodesWalk<true> nd;
    const int nq = step128(n);
    nd.start(nodes, rb, g * RPG + l);
    uint64_t t0 = 0, t1 = 0;   // an adjacency without tiles may come without row_ptr
    if (n_tiles != 0 && nd.block_live()) {
        t0 = static_cast<uint64_t>(row_ptr[rb]);
        t1 = static_cast<uint64_t>(row_ptr[rb + 1]);
        t1 = t1 < n_tiles ? t1 : n_tiles;
    }
    TiledU8Weighted red[RPG];
    int cnt[RPG];
#pragma unroll
    for (int ri = 0; ri < RPG; ++ri) {
        cnt[ri] = 0;
        red[ri].reset();
    }
    const bool loader = l < RPG && nd.row_live();                  // lane l < RPG: row g * RPG + l of every tile
    const int my_row = g * RPG + (l < RPG ? l : 0);
    const uint32_t *mine = tiles + my_row * 4;
    uint4 a = make_uint4(0, 0, 0, 0);
    int q = -1, vp = 0, vr = 0;   // val_ptr of the tile being decoded; a loader lane: val_row of its row of that tile
    if (t0 < t1) {
        q = kquad[t0];
        vp = static_cast<int>(ed.val_ptr[t0]);
        if (loader) {
            a = *reinterpret_cast<const uint4 *>(mine + t0 * 128);
            vr = ed.val_row[t0 * 32 + my_row];
        }
        nd.load(nd.nb, q, nq);
    }
    for (uint64_t t = t0; t < t1; ++t) {
        uint4 an = make_uint4(0, 0, 0, 0);
        int qn = -1, vpn = 0, vrn = 0;
        if (t + 1 < t1) {
            qn = kquad[t + 1];
            vpn = static_cast<int>(ed.val_ptr[t + 1]);
            if (loader) {
                an = *reinterpret_cast<const uint4 *>(mine + (t + 1) * 128);
                vrn = ed.val_row[(t + 1) * 32 + my_row];
            }
            nd.load(nd.nbn, qn, nq);
        }
        if (static_cast<unsigned>(q) < static_cast<unsigned>(nq) && nd.tile_live()) {
            const uint32_t w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
            for (int ri = 0; ri < RPG; ++ri) {
                int sb = vp + static_cast<int>(tiled_u8_bcast<LPR>(static_cast<uint32_t>(vr), ri));   // the slot of the row's next raw bit
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t raw = tiled_u8_bcast<LPR>(w[k], ri);
                    tiled_u8e_decode_row(raw & nd.word(k), raw, sb, q * 128 + k * 32, n, red[ri], lists[g][ri], slots[g][ri], cnt[ri], Q, ld,
                                         cb, mine_cols, e);
                    sb += __builtin_popcount(raw);
                }
            }
        }
        a = an;
        q = qn;
        vp = vpn;
        vr = vrn;
        nd.nb = nd.nbn;
    }
#pragma unroll
    for (int ri = 0; ri < RPG; ++ri) {
        tiled_u8e_fold(red[ri], lists[g][ri], slots[g][ri], cnt[ri], Q, ld, cb, mine_cols, e);
        const int row = rb * 32 + g * RPG + ri;
        if (row < n) tiled_u8e_store<CODES>(red[ri], row, cb, N, qp, row_scale, out);
    }
}

// ---- the column view ---------------------------------------------------------------------------------------------------------------------
// tiled_u8_col_walk with slots. The transposer role keeps, beside the transposed masks of a round's 8 tiles, their RAW words
// (8 x 32 rows x 4 words), every row's val_row and every tile's val_ptr in LDS, all loaded one round ahead with the words: a column mask
// does not say what lies left of a cell in its tile row. Between rounds the state of the 128 x 4 LPR outputs is a float4 a lane and
// output row and one float (sum w of the lane's head) beside it.
template <int LPR, bool CODES>
__global__ __launch_bounds__(256) void k_tiled_mm_u8_t_edge(const int64_t *__restrict__ col_ptr, const int64_t *__restrict__ col_tile,
                                                            const int32_t *__restrict__ col_rb, const uint32_t *__restrict__ tiles,
                                                            uint64_t n_tiles, int n, const uint8_t *__restrict__ Q, size_t ld, int N,
                                                            const float4 *__restrict__ qp, const float *__restrict__ row_scale,
                                                            TiledU8Edge ed, TiledU8EdgeOut out, TiledNodes nodes) {
    constexpr int G = 256 / LPR, TS = TILED_T_TS;
    static_assert(TS == 8, "an output row reads its 8 masks of a round as two uint4");
    __shared__ __attribute__((aligned(16))) uint32_t mk[128 * TS];        // [tile column][staged tile]
    __shared__ __attribute__((aligned(16))) uint32_t raw[TS * 32 * 4];   // [staged tile][tile row][word], as stored
    __shared__ int srb[TS], evp[TS], evr[TS * 32];                        // the staged tiles' row blocks, val_ptr and val_row
    __shared__ __attribute__((aligned(16))) float acc[128 * LPR * 4];    // [output row][lane][4 columns]: sum w q
    __shared__ float asw[128 * LPR];                                      // [output row][lane]: sum w of the lane's head
    __shared__ int lists[G][TILED_U8_CAP], slots[G][TILED_U8_CAP];
    const int q = blockIdx.x, tid = threadIdx.x;
    const int g = LPR == 64 ? __builtin_amdgcn_readfirstlane(tid / LPR) : tid / LPR;
    const int l = tid % LPR, cb = blockIdx.y * (LPR * 4) + l * 4;
    const bool mine_cols = cb < N;
    const TiledU8EdgeLane e = tiled_u8e_lane(ed, cb, N);
    const int nrb = (n + 31) / 32;
    float4 *acc4 = reinterpret_cast<float4 *>(acc);
    for (int j = g; j < 128; j += G) {
        acc4[j * LPR + l] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        asw[j * LPR + l] = 0.0f;
    }

    const int lane = tid & 31, s_own = tid >> 5;   // transposer role: half-wave s of the workgroup stages tile base + s
    uint64_t b0 = 0, t1 = 0;                       // an adjacency without tiles may come without col_ptr
    const uint4 rw = tiled_nodes_quad(nodes.row, q);   // the row bitmap's words of this k-quad
    if (n_tiles != 0 && (rw.x | rw.y | rw.z | rw.w) != 0) {
        b0 = static_cast<uint64_t>(col_ptr[q]);
        t1 = static_cast<uint64_t>(col_ptr[q + 1]);
        t1 = t1 < n_tiles ? t1 : n_tiles;
    }
    auto entry = [&](uint64_t i, uint64_t &t, int &rb) {
        t = n_tiles;
        rb = -1;
        if (i < t1) {
            t = static_cast<uint64_t>(col_tile[i]);
            rb = col_rb[i];
        }
    };
    // this lane's tile row 31 - lane: its words as stored (`r4`), its val_row and the tile's val_ptr, and the words under both bitmaps
    // (returned). A skipped tile or row block, and a tile without a live neighbour, leave zero masks: their raw words are never looked at.
    uint4 r4;
    int vr, vp;
    auto words = [&](uint64_t t, int &rb) {
        r4 = make_uint4(0, 0, 0, 0);
        vr = vp = 0;
        if (t < n_tiles && static_cast<unsigned>(rb) < static_cast<unsigned>(nrb)) {
            const uint32_t nb = nodes.nbr ? nodes.nbr[rb] : 0xffffffffu;   // rb < S32(n) <= S128(n) * 4
            if (nb) {
                r4 = *reinterpret_cast<const uint4 *>(tiles + t * 128 + (31 - lane) * 4);
                vr = ed.val_row[t * 32 + (31 - lane)];
                vp = static_cast<int>(ed.val_ptr[t]);
                const uint32_t on = (nb >> lane) & 1u ? 0xffffffffu : 0u;   // lane holds tile row 31 - lane: bit `lane` of the word
                return make_uint4(r4.x & rw.x & on, r4.y & rw.y & on, r4.z & rw.z & on, r4.w & rw.w & on);
            }
        }
        rb = -1;
        return make_uint4(0, 0, 0, 0);
    };
    uint4 w;
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
            *reinterpret_cast<uint4 *>(raw + (s_own * 32 + 31 - lane) * 4) = r4;
            evr[s_own * 32 + 31 - lane] = vr;
            tiled_t_transpose(v, lane);
#pragma unroll
            for (int k = 0; k < 4; ++k) mk[(k * 32 + 31 - lane) * TS + s_own] = v[k];
            if (lane == 0) {
                srb[s_own] = rb;
                evp[s_own] = vp;
            }
            rb = rbn;
            w = words(tn, rb);
            entry(base + 2 * TS + s_own, tn, rbn);
        }
        __syncthreads();
        for (int j = g; j < 128; j += G) {
            if (q * 128 + j >= n) break;
            const uint4 ma = *reinterpret_cast<const uint4 *>(mk + j * TS), mb = *reinterpret_cast<const uint4 *>(mk + j * TS + 4);
            const uint32_t m[TS] = {ma.x, ma.y, ma.z, ma.w, mb.x, mb.y, mb.z, mb.w};
            if (!(ma.x | ma.y | ma.z | ma.w | mb.x | mb.y | mb.z | mb.w)) continue;
            const float4 s4 = acc4[j * LPR + l];
            TiledU8Weighted r{tiled_u8e_f2{s4.x, s4.y}, tiled_u8e_f2{s4.z, s4.w}, asw[j * LPR + l]};
            int cnt = 0;
#pragma unroll
            for (int st = 0; st < TS; ++st)
                if (m[st])
                    tiled_u8e_decode_col(m[st], raw + st * 128, evr + st * 32, evp[st], j, srb[st] * 32, n, r, lists[g], slots[g], cnt, Q, ld, cb,
                                         mine_cols, e);
            tiled_u8e_fold(r, lists[g], slots[g], cnt, Q, ld, cb, mine_cols, e);
            acc4[j * LPR + l] = make_float4(r.lo.x, r.lo.y, r.hi.x, r.hi.y);
            asw[j * LPR + l] = r.sw;
        }
        __syncthreads();
    }

    for (int j = g; j < 128; j += G) {
        const int row = q * 128 + j;
        if (row >= n) break;
        const float4 s4 = acc4[j * LPR + l];
        tiled_u8e_store<CODES>(TiledU8Weighted{tiled_u8e_f2{s4.x, s4.y}, tiled_u8e_f2{s4.z, s4.w}, asw[j * LPR + l]}, row, cb, N, qp, row_scale,
                               out);
    }
}

// the family as tiled_u8_launch takes it; its tail is (const float4 *qp, const float *row_scale, TiledU8Edge ed, TiledU8EdgeOut out). The
// column view's state is 20 bytes a lane and output row: 80 KiB at 32 lanes, so 32 is its widest class.
template <bool CODES>
struct TiledU8EdgeKernels {
    static constexpr int COL_WIDEST = 32;
    template <int LPR> static auto row() { return k_tiled_mm_u8_edge<LPR, CODES>; }
    template <int LPR> static auto col() { return k_tiled_mm_u8_t_edge<LPR, CODES>; }
};

// ---- the entries' body, either view: invalid, then misaligned, then short (merged with the value index's), then the launch ------------
template <class Index>
int tiled_u8_edge_entry(const Index &ix, const TiledU8In &a, const float *qparams, const float *row_scale, const int64_t *val_ptr,
                        const int16_t *val_row, const float *values, size_t n_values, int heads, const CodesDest &d, void *stream) {
    int own = QGTC_OK;
    if (tiled_u8_invalid(ix, a) || codes_dest_invalid(d) || !qparams || heads < 1 || a.N % heads != 0 ||
        (heads > 1 && (a.N / heads) % 4 != 0) || (a.n_tiles > 0 && !values))
        own = QGTC_EINVAL;
    else if (tiled_u8_misaligned(a) || codes_dest_misaligned(d, a.N) || !aligned16(qparams) || !codes_aligned4(row_scale) ||
             !codes_aligned4(values))
        own = QGTC_EALIGN;
    else if (tiled_u8_short(a) || codes_dest_short(d, a.n, a.N))
        own = QGTC_ESIZE;
    const int rc = tiled_edge_rc(own, tiled_edge_index_ok(val_ptr, val_row, a.n_tiles, n_values));
    if (rc != QGTC_OK) return rc;
    const float4 *qp = reinterpret_cast<const float4 *>(qparams);
    const TiledU8Edge ed{val_ptr, val_row, values, static_cast<int>(n_values), heads};
    if (d.out) return tiled_u8_launch<TiledU8EdgeKernels<false>>(ix, a, stream, qp, row_scale, ed, TiledU8EdgeOut{d.out, 0, nullptr, 0.0f});
    return tiled_u8_launch<TiledU8EdgeKernels<true>>(ix, a, stream, qp, row_scale, ed, TiledU8EdgeOut{d.outq, d.ldo, d.qp(), d.qmax()});
}

}  // namespace
