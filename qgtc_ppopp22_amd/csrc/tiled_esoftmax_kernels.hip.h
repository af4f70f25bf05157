// tiled_esoftmax_kernels.hip.h — part of libqgtc_hip.so (included by qgtc_tiled_esoftmax.hip and qgtc_tiled_esoftmax_t.hip, after
// tiled_float_kernels.hip.h, tiled_max_kernels.hip.h and tiled_attn_kernels.hip.h and before tiled_heads_esoftmax_kernels.hip.h,
// which has the kernels for H heads and the host side of both; the column view's unit defines QGTC_TILED_ESOFTMAX_T and includes
// tiled_t_kernels.hip.h first): the softmax of a vector of per-edge logits over each node's neighbourhood on the tile-compressed
// adjacency, and its gradient (include/qgtc.h, "Edge softmax"). Logits, weights and gradients are float32
// [n_values] in SLOT order (tiled_edge.hip.h), one array for both views.
//
// A lane owns one node - a row on the row view, a column on the column view - and visits that node's cells in ascending id of the other
// end, so every fold is the in-order one of the contract and no lane reads what another produced:
//   forward   three walks: m = the first maximum of the logits; den = the fold of w = EXP(fl(l - m)); alpha = fl(w * inv), w recomputed;
//   gradient  two walks: S = the fold of fl(alpha * g); out = fl(alpha * fl(g - S)).
// A walk is written once per view and takes a PASS: load(slot) reads what the pass needs of a cell, apply(slot, value) folds or stores.
// Row view: a workgroup of 256 lanes covers 8 row blocks; lane r of a block reads row r of each of the block's tiles (16 bytes, the
// block's 32 lanes read the tile's 512 bytes together), and the row's cells are the contiguous slots from val_ptr[t] + val_row[t][r];
// the next tile's words are loaded while this one's cells are visited.
// Column view: a workgroup of 128 lanes per k-quad, lane j on column j. The k-quad's column list is walked TS = 8 tiles a round in
// ascending tile order (= ascending row block). As in k_tiled_mm_f32_t each half-wave is a transposer: it loads a tile (two a round),
// keeps the raw words, val_row and val_ptr in LDS and runs the 32 x 32 bit transpose, so that a lane reads its column's masks of the
// round as two 16-byte words; the next round's loads are issued before this round is decoded. A column's cells lie in different tile
// rows, so their slots are scattered: a lane queues the slots (tiled_edge_row_before on the staged row) in a lane-private strip of LDS
// and, CAP at a time, issues the loads together before it folds them in order - one memory latency a batch instead of one a cell.
// A slot outside [0, n_values) is never dereferenced (the cell is skipped); rows and columns at or past n are masked out. Every float
// operation goes through a helper under `fp contract(off)`.
#pragma once

namespace {

__device__ __forceinline__ float tiled_esm_add(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}

// the statistics of one owner, filled by the passes in this order
struct TiledEsmFwd {
    const float *__restrict__ logits;
    float *__restrict__ alpha;
    float m, den, inv;
    bool first;
    __device__ __forceinline__ float weight(float l) const { return tiled_att_exp(tiled_att_sub(l, m)); }
    __device__ __forceinline__ void finish() { inv = den > 0.0f ? __fdiv_rn(1.0f, den) : 0.0f; }   // the attention forward's expression
};
struct TiledEsmMaxPass {
    TiledEsmFwd &st;
    using V = float;
    __device__ __forceinline__ V load(int s) const { return st.logits[s]; }
    __device__ __forceinline__ void apply(int, V l) {
        st.m = st.first ? l : (l > st.m ? l : st.m);   // the first of equal values wins
        st.first = false;
    }
};
struct TiledEsmDenPass {
    TiledEsmFwd &st;
    using V = float;
    __device__ __forceinline__ V load(int s) const { return st.logits[s]; }
    __device__ __forceinline__ void apply(int, V l) { st.den = tiled_esm_add(st.den, st.weight(l)); }
};
struct TiledEsmAlphaPass {
    TiledEsmFwd &st;
    using V = float;
    __device__ __forceinline__ V load(int s) const { return st.logits[s]; }
    __device__ __forceinline__ void apply(int s, V l) { st.alpha[s] = tiled_att_mul(st.weight(l), st.inv); }
};

struct TiledEsmBwd {
    const float *__restrict__ alpha;
    const float *__restrict__ g;
    float *__restrict__ out;
    float S;
};
struct TiledEsmSumPass {
    TiledEsmBwd &st;
    using V = float2;
    __device__ __forceinline__ V load(int s) const { return make_float2(st.alpha[s], st.g[s]); }
    __device__ __forceinline__ void apply(int, V v) { st.S = tiled_esm_add(st.S, tiled_att_mul(v.x, v.y)); }
};
struct TiledEsmOutPass {
    TiledEsmBwd &st;
    using V = float2;
    __device__ __forceinline__ V load(int s) const { return make_float2(st.alpha[s], st.g[s]); }
    __device__ __forceinline__ void apply(int s, V v) { st.out[s] = tiled_att_mul(v.x, tiled_att_sub(v.y, st.S)); }
};

// the top `left` bits of a word (element i at bit 31 - i): the elements of the word that lie below n
__device__ __forceinline__ uint32_t tiled_esm_keep(int left) {
    return left >= 32 ? 0xffffffffu : left <= 0 ? 0u : 0xffffffffu << (32 - left);
}

#ifndef QGTC_TILED_ESOFTMAX_T
// ---- the row view -----------------------------------------------------------------------------------------------------------------------
// the pass over the cells of row r of the tiles t0 .. t1 - 1 of one row block, in ascending column order
template <class P>
__device__ __forceinline__ void tiled_esm_row_walk(const int32_t *__restrict__ kquad, const uint32_t *__restrict__ tiles,
                                                   const int64_t *__restrict__ val_ptr, const int16_t *__restrict__ val_row, uint64_t t0,
                                                   uint64_t t1, int r, int n, int n_values, P p) {
    const int nq = step128(n);
    uint4 a = make_uint4(0, 0, 0, 0);
    int q = -1, s0 = 0;
    auto load = [&](uint64_t t, uint4 &w, int &qq, int &ss) {
        qq = kquad[t];
        w = *reinterpret_cast<const uint4 *>(tiles + t * 128 + r * 4);
        ss = static_cast<int>(val_ptr[t]) + val_row[t * 32 + r];
    };
    if (t0 < t1) load(t0, a, q, s0);
    for (uint64_t t = t0; t < t1; ++t) {
        uint4 an = make_uint4(0, 0, 0, 0);
        int qn = -1, sn = 0;
        if (t + 1 < t1) load(t + 1, an, qn, sn);
        if (static_cast<unsigned>(q) < static_cast<unsigned>(nq)) {
            const int left = n - q * 128;
            const int cnt = __builtin_popcount(a.x & tiled_esm_keep(left)) + __builtin_popcount(a.y & tiled_esm_keep(left - 32)) +
                            __builtin_popcount(a.z & tiled_esm_keep(left - 64)) + __builtin_popcount(a.w & tiled_esm_keep(left - 96));
            for (int i = 0; i < cnt; ++i) {
                const int s = s0 + i;
                if (static_cast<unsigned>(s) < static_cast<unsigned>(n_values)) p.apply(s, p.load(s));
            }
        }
        a = an;
        q = qn;
        s0 = sn;
    }
}

// the tile range of the row of this lane and whether the lane has a row at all
struct TiledEsmRow {
    uint64_t t0, t1;
    int row, r;
    bool live;
};
__device__ __forceinline__ TiledEsmRow tiled_esm_row_of(const int64_t *__restrict__ row_ptr, uint64_t n_tiles, int n) {
    TiledEsmRow w{0, 0, 0, 0, false};
    const int rb = blockIdx.x * 8 + static_cast<int>(threadIdx.x) / 32;
    w.r = threadIdx.x % 32;
    w.row = rb * 32 + w.r;
    w.live = w.row < n;
    if (w.live && n_tiles != 0) {   // an adjacency without tiles may come without row_ptr
        w.t0 = static_cast<uint64_t>(row_ptr[rb]);
        w.t1 = static_cast<uint64_t>(row_ptr[rb + 1]);
        w.t1 = w.t1 < n_tiles ? w.t1 : n_tiles;
    }
    return w;
}

__global__ __launch_bounds__(256) void k_tiled_esoftmax(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ kquad,
                                                        const uint32_t *__restrict__ tiles, uint64_t n_tiles, int n,
                                                        const int64_t *__restrict__ val_ptr, const int16_t *__restrict__ val_row,
                                                        const float *__restrict__ logits, float *__restrict__ alpha, int n_values,
                                                        float *__restrict__ m_out, float *__restrict__ inv_out) {
    const TiledEsmRow w = tiled_esm_row_of(row_ptr, n_tiles, n);
    if (!w.live) return;
    TiledEsmFwd st{logits, alpha, 0.0f, 0.0f, 0.0f, true};
    tiled_esm_row_walk(kquad, tiles, val_ptr, val_row, w.t0, w.t1, w.r, n, n_values, TiledEsmMaxPass{st});
    tiled_esm_row_walk(kquad, tiles, val_ptr, val_row, w.t0, w.t1, w.r, n, n_values, TiledEsmDenPass{st});
    st.finish();
    tiled_esm_row_walk(kquad, tiles, val_ptr, val_row, w.t0, w.t1, w.r, n, n_values, TiledEsmAlphaPass{st});
    if (m_out) m_out[w.row] = st.m;
    if (inv_out) inv_out[w.row] = st.inv;
}

__global__ __launch_bounds__(256) void k_tiled_esoftmax_grad(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ kquad,
                                                             const uint32_t *__restrict__ tiles, uint64_t n_tiles, int n,
                                                             const int64_t *__restrict__ val_ptr, const int16_t *__restrict__ val_row,
                                                             const float *__restrict__ alpha, const float *__restrict__ g,
                                                             float *__restrict__ out, int n_values) {
    const TiledEsmRow w = tiled_esm_row_of(row_ptr, n_tiles, n);
    if (!w.live) return;
    TiledEsmBwd st{alpha, g, out, 0.0f};
    tiled_esm_row_walk(kquad, tiles, val_ptr, val_row, w.t0, w.t1, w.r, n, n_values, TiledEsmSumPass{st});
    tiled_esm_row_walk(kquad, tiles, val_ptr, val_row, w.t0, w.t1, w.r, n, n_values, TiledEsmOutPass{st});
}

#else
// ---- the column view --------------------------------------------------------------------------------------------------------------------
constexpr int TILED_ESM_TS = TILED_T_TS;   // tiles staged per round
constexpr int TILED_ESM_CAP = 16;          // slots a lane queues before it loads and folds them

// what a workgroup keeps in LDS: a round's raw tile words (four a row), the column masks after the transpose ([tile column][staged
// tile]), the tiles' in-tile row prefix, val_ptr and row block (-1: the list entry is skipped), and the lanes' slot queues ([entry][lane])
struct TiledEsmStage {
    __attribute__((aligned(16))) uint32_t raw[TILED_ESM_TS * 128];
    __attribute__((aligned(16))) uint32_t mk[128 * TILED_ESM_TS];
    int vrow[TILED_ESM_TS * 32];
    int vp[TILED_ESM_TS], rb[TILED_ESM_TS];
    int queue[TILED_ESM_CAP * 128];
};

// the pass over the first cnt (1 .. CAP) queued slots of lane j: the loads are issued together, then applied in order
template <class P>
__device__ __forceinline__ void tiled_esm_flush(const int *queue, int j, int cnt, P &p) {
    typename P::V v[TILED_ESM_CAP];
    int s[TILED_ESM_CAP];
#pragma unroll
    for (int i = 0; i < TILED_ESM_CAP; ++i) {
        s[i] = queue[(i < cnt ? i : cnt - 1) * 128 + j];
        v[i] = p.load(s[i]);
    }
#pragma unroll
    for (int i = 0; i < TILED_ESM_CAP; ++i)
        if (i < cnt) p.apply(s[i], v[i]);
}

// the pass over the cells of column j (0 .. 127) of the tiles listed at b0 .. t1 - 1, in ascending row order. Every lane of the
// workgroup (128) calls it with the same list: the barriers are inside. `live` false: the lane stages tiles and visits nothing.
template <class P>
__device__ __forceinline__ void tiled_esm_col_walk(const int64_t *__restrict__ col_tile, const int32_t *__restrict__ col_rb,
                                                   const uint32_t *__restrict__ tiles, uint64_t n_tiles, int n,
                                                   const int64_t *__restrict__ val_ptr, const int16_t *__restrict__ val_row, uint64_t b0,
                                                   uint64_t t1, int j, bool live, int n_values, TiledEsmStage &lds, P p) {
    constexpr int TS = TILED_ESM_TS;
    static_assert(TS == 8, "a column reads its 8 masks of a round as two uint4; a half-wave stages two tiles a round");
    const int tid = threadIdx.x, lane = tid & 31, h = tid >> 5, nrb = (n + 31) / 32;
    // transposer role: half-wave h stages the tiles h and h + 4 of a round, lane l their row 31 - l
    uint4 w[2];
    int rb[2], vr[2], vp[2];
    auto fetch = [&](uint64_t base) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const uint64_t i = base + h + 4 * u;
            w[u] = make_uint4(0, 0, 0, 0);
            rb[u] = -1;
            vr[u] = vp[u] = 0;
            if (i < t1) {
                const uint64_t t = static_cast<uint64_t>(col_tile[i]);
                const int r = col_rb[i];
                if (t < n_tiles && static_cast<unsigned>(r) < static_cast<unsigned>(nrb)) {
                    w[u] = *reinterpret_cast<const uint4 *>(tiles + t * 128 + (31 - lane) * 4);
                    vr[u] = val_row[t * 32 + 31 - lane];
                    vp[u] = static_cast<int>(val_ptr[t]);
                    rb[u] = r;
                }
            }
        }
    };
    int cnt = 0;
    if (b0 < t1) fetch(b0);
    for (uint64_t base = b0; base < t1; base += TS) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int s = h + 4 * u;
            *reinterpret_cast<uint4 *>(lds.raw + (s * 32 + 31 - lane) * 4) = w[u];
            lds.vrow[s * 32 + 31 - lane] = vr[u];
            uint32_t v[4] = {w[u].x, w[u].y, w[u].z, w[u].w};
            tiled_t_transpose(v, lane);
#pragma unroll
            for (int k = 0; k < 4; ++k) lds.mk[(k * 32 + 31 - lane) * TS + s] = v[k];
            if (lane == 0) {
                lds.rb[s] = rb[u];
                lds.vp[s] = vp[u];
            }
        }
        if (base + TS < t1) fetch(base + TS);   // in flight while this round is decoded
        __syncthreads();
        if (live) {
            const uint4 ma = *reinterpret_cast<const uint4 *>(lds.mk + j * TS), mb = *reinterpret_cast<const uint4 *>(lds.mk + j * TS + 4);
            const uint32_t m[TS] = {ma.x, ma.y, ma.z, ma.w, mb.x, mb.y, mb.z, mb.w};
            if (ma.x | ma.y | ma.z | ma.w | mb.x | mb.y | mb.z | mb.w) {
#pragma unroll
                for (int st = 0; st < TS; ++st) {
                    if (!m[st]) continue;
                    uint32_t mask = m[st] & tiled_esm_keep(n - lds.rb[st] * 32);   // source rows at or past n are masked out
                    const uint32_t *raw = lds.raw + st * 128;
                    const int vbase = lds.vp[st];
                    while (mask) {
                        const int b = __builtin_clz(mask);
                        mask &= ~(0x80000000u >> b);
                        const uint32_t *r = raw + b * 4;
                        const int sl = vbase + lds.vrow[st * 32 + b] + tiled_edge_row_before(r[0], r[1], r[2], r[3], j);
                        if (static_cast<unsigned>(sl) < static_cast<unsigned>(n_values)) {
                            lds.queue[cnt * 128 + j] = sl;
                            if (++cnt == TILED_ESM_CAP) {
                                tiled_esm_flush(lds.queue, j, cnt, p);
                                cnt = 0;
                            }
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
    if (live && cnt) tiled_esm_flush(lds.queue, j, cnt, p);
}

struct TiledEsmCol {
    uint64_t b0, t1;
    int col, j;
    bool live;
};
__device__ __forceinline__ TiledEsmCol tiled_esm_col_of(const int64_t *__restrict__ col_ptr, uint64_t n_tiles, int n) {
    TiledEsmCol w{0, 0, 0, 0, false};
    const int q = blockIdx.x;
    w.j = threadIdx.x;
    w.col = q * 128 + w.j;
    w.live = w.col < n;
    if (n_tiles != 0) {   // the whole workgroup takes the same list; an adjacency without tiles may come without col_ptr
        w.b0 = static_cast<uint64_t>(col_ptr[q]);
        w.t1 = static_cast<uint64_t>(col_ptr[q + 1]);
        w.t1 = w.t1 < n_tiles ? w.t1 : n_tiles;
    }
    return w;
}

__global__ __launch_bounds__(128) void k_tiled_esoftmax_t(const int64_t *__restrict__ col_ptr, const int64_t *__restrict__ col_tile,
                                                          const int32_t *__restrict__ col_rb, const uint32_t *__restrict__ tiles,
                                                          uint64_t n_tiles, int n, const int64_t *__restrict__ val_ptr,
                                                          const int16_t *__restrict__ val_row, const float *__restrict__ logits,
                                                          float *__restrict__ alpha, int n_values, float *__restrict__ m_out,
                                                          float *__restrict__ inv_out) {
    __shared__ TiledEsmStage lds;
    const TiledEsmCol w = tiled_esm_col_of(col_ptr, n_tiles, n);
    TiledEsmFwd st{logits, alpha, 0.0f, 0.0f, 0.0f, true};
    tiled_esm_col_walk(col_tile, col_rb, tiles, n_tiles, n, val_ptr, val_row, w.b0, w.t1, w.j, w.live, n_values, lds, TiledEsmMaxPass{st});
    tiled_esm_col_walk(col_tile, col_rb, tiles, n_tiles, n, val_ptr, val_row, w.b0, w.t1, w.j, w.live, n_values, lds, TiledEsmDenPass{st});
    st.finish();
    tiled_esm_col_walk(col_tile, col_rb, tiles, n_tiles, n, val_ptr, val_row, w.b0, w.t1, w.j, w.live, n_values, lds, TiledEsmAlphaPass{st});
    if (w.live) {
        if (m_out) m_out[w.col] = st.m;
        if (inv_out) inv_out[w.col] = st.inv;
    }
}

__global__ __launch_bounds__(128) void k_tiled_esoftmax_grad_t(const int64_t *__restrict__ col_ptr, const int64_t *__restrict__ col_tile,
                                                               const int32_t *__restrict__ col_rb, const uint32_t *__restrict__ tiles,
                                                               uint64_t n_tiles, int n, const int64_t *__restrict__ val_ptr,
                                                               const int16_t *__restrict__ val_row, const float *__restrict__ alpha,
                                                               const float *__restrict__ g, float *__restrict__ out, int n_values) {
    __shared__ TiledEsmStage lds;
    const TiledEsmCol w = tiled_esm_col_of(col_ptr, n_tiles, n);
    TiledEsmBwd st{alpha, g, out, 0.0f};
    tiled_esm_col_walk(col_tile, col_rb, tiles, n_tiles, n, val_ptr, val_row, w.b0, w.t1, w.j, w.live, n_values, lds, TiledEsmSumPass{st});
    tiled_esm_col_walk(col_tile, col_rb, tiles, n_tiles, n, val_ptr, val_row, w.b0, w.t1, w.j, w.live, n_values, lds, TiledEsmOutPass{st});
}
#endif

}  // namespace
