// tiled_codes_walk.hip.h — part of libqgtc_hip.so (included by tiled_codes_kernels.hip.h, after common.hip.h and bitmm_popcount.hip.h):
// the tile walk of the byte-code family, written once per view, with what is reduced as a policy. The fused
// middle of tiled_codes_linear_kernels.hip.h and the extremum of tiled_codes_max_kernels.hip.h are this walk with a reducer; a kernel
// adds its setup and its epilogue. The two sum kernels of tiled_codes_kernels.hip.h keep a walk of their own (6.15u says why).
//
// The walks are those of k_tiled_mm_f32 and k_tiled_mm_f32_t: a tile's set bits are decoded MSB first into an LDS queue of TILED_U8_CAP
// ids and the addressed rows of the operand are loaded TILED_U8_AHEAD at a time. What differs: a lane owns FOUR ADJACENT columns and
// loads one dword per neighbour row (hence ld % 4 == 0); a lane whose columns all lie past N loads nothing, a dword that straddles N is
// loaded and its surplus bytes are not stored. The node masks are always compiled in (either pointer may be null: all nodes).
//
// A reducer is a lane's state for one output row and what is done to it:
//   reset()                             the state of a row without a term
//   note()                              an id was queued for the row
//   fold(list, cnt, Q, ld, cb, mine)    reduce Q[list[j]][cb .. cb + 3], j < cnt, into the state, TILED_U8_AHEAD loads at a time
//   Acc, fetch / put(acc, aux, slot, j) the column view's state in LDS between rounds: the lane's part at acc[slot], the row's at aux[j]
//                                       (every lane of the group writes it: the same value); only a reducer used on that view has them
#pragma once

#include "tiled_args.hip.h"
#include "tiled_nodes.hip.h"
#include "tiled_t_kernels.hip.h"   // the in-register bit transpose of the column view

namespace {

constexpr int TILED_U8_CAP = 32;    // decoded neighbour ids a row group queues in LDS before it reduces their rows
constexpr int TILED_U8_AHEAD = 4;   // rows of Q whose loads are in flight before the first of them is reduced

// s[k] += Q[list[j]][cb + k], k < 4, j < cnt. TILED_U8_AHEAD loads are issued together (past the end the last entry is loaded again and
// not added). `mine`: the lane's first column lies inside N, else it loads nothing. `list`: LDS, every lane wrote every entry itself.
__device__ __forceinline__ void tiled_u8_add_rows(int (&s)[4], const int *list, int cnt, const uint8_t *__restrict__ Q, size_t ld, int cb,
                                                  bool mine) {
#pragma nounroll
    for (int j = 0; j < cnt; j += TILED_U8_AHEAD) {
        uint32_t w[TILED_U8_AHEAD];
#pragma unroll
        for (int u = 0; u < TILED_U8_AHEAD; ++u) {
            const int v = list[j + u < cnt ? j + u : cnt - 1];
            w[u] = mine ? *reinterpret_cast<const uint32_t *>(Q + static_cast<size_t>(v) * ld + cb) : 0u;
        }
#pragma unroll
        for (int u = 0; u < TILED_U8_AHEAD; ++u)
            if (j + u < cnt) {
                s[0] += static_cast<int>(w[u] & 0xffu);
                s[1] += static_cast<int>((w[u] >> 8) & 0xffu);
                s[2] += static_cast<int>((w[u] >> 16) & 0xffu);
                s[3] += static_cast<int>(w[u] >> 24);
            }
    }
}

// ---- the sum: s[k] += Q[v][cb + k], and the terms of the row ---------------------------------------------------------------------------
// int32 sums, one register per column, each byte added to its own (v_add_u32_sdwa with a BYTE_k source):
// exact in any order, so only the loads need run ahead. `terms` is the degree under the masks, which the affine epilogue needs.
struct TiledU8Sum {
    int s[4], terms;
    __device__ __forceinline__ void reset() {
        terms = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] = 0;
    }
    __device__ __forceinline__ void note() { ++terms; }
    __device__ __forceinline__ void fold(const int *list, int cnt, const uint8_t *__restrict__ Q, size_t ld, int cb, bool mine) {
        tiled_u8_add_rows(s, list, cnt, Q, ld, cb, mine);
    }
};

// ---- the extremum: s = bytewise max(s, Q[v][cb .. cb + 3] ^ flip), and whether the row had a term ---------------------------------------
// ONE packed dword per output row: the byte-wise maximum is taken on even and odd bytes as two packed 16-bit maxima (v_pk_max_u16), the
// halves split once when a queue is drained and joined once after it. Min is max on complemented bytes: every loaded dword is XORed with
// `flip` (0, or 0xffffffff for min) and XORed back by the epilogue, so the identity is 0 either way. A maximum is idempotent: the
// load-ahead's surplus slots are reduced like any other. There is no term count, only `had`: an extremum over nothing has no value.
typedef unsigned short tiled_max_u16x2 __attribute__((ext_vector_type(2)));

struct TiledU8Extremum {
    using Acc = uint32_t;
    uint32_t s, flip;
    bool had;
    __device__ __forceinline__ void reset() {
        s = 0;
        had = false;
    }
    __device__ __forceinline__ void note() { had = true; }
    __device__ __forceinline__ void fold(const int *list, int cnt, const uint8_t *__restrict__ Q, size_t ld, int cb, bool mine) {
        tiled_max_u16x2 ev = __builtin_bit_cast(tiled_max_u16x2, s & 0x00ff00ffu), od = __builtin_bit_cast(tiled_max_u16x2, (s >> 8) & 0x00ff00ffu);
#pragma nounroll
        for (int j = 0; j < cnt; j += TILED_U8_AHEAD) {
            uint32_t w[TILED_U8_AHEAD];
#pragma unroll
            for (int u = 0; u < TILED_U8_AHEAD; ++u) {
                const int v = list[j + u < cnt ? j + u : cnt - 1];
                w[u] = mine ? *reinterpret_cast<const uint32_t *>(Q + static_cast<size_t>(v) * ld + cb) ^ flip : 0u;
            }
#pragma unroll
            for (int u = 0; u < TILED_U8_AHEAD; ++u) {
                ev = __builtin_elementwise_max(ev, __builtin_bit_cast(tiled_max_u16x2, w[u] & 0x00ff00ffu));
                od = __builtin_elementwise_max(od, __builtin_bit_cast(tiled_max_u16x2, (w[u] >> 8) & 0x00ff00ffu));
            }
        }
        s = __builtin_bit_cast(uint32_t, ev) | (__builtin_bit_cast(uint32_t, od) << 8);
    }
    __device__ __forceinline__ void fetch(const uint32_t *acc, const int *any, int slot, int j) {
        s = acc[slot];
        had = any[j] != 0;
    }
    __device__ __forceinline__ void put(uint32_t *acc, int *any, int slot, int j) const {
        acc[slot] = s;
        any[j] = had;
    }
};

// the set bits of `m`, MSB first, as ids base + (leading zeros), queued and noted; ids from n up are dropped (a foreign tile must not
// make the kernel read past Q). A full queue is reduced at once.
template <class R>
__device__ __forceinline__ void tiled_u8_decode(uint32_t m, int base, int n, R &r, int *list, int &cnt, const uint8_t *__restrict__ Q,
                                                size_t ld, int cb, bool mine) {
    while (m) {
        const int b = __builtin_clz(m);
        m &= ~(0x80000000u >> b);
        const int v = base + b;
        if (v < n) {
            list[cnt++] = v;
            r.note();
            if (cnt == TILED_U8_CAP) {
                r.fold(list, cnt, Q, ld, cb, mine);
                cnt = 0;
            }
        }
    }
}

template <int LPR>
__device__ __forceinline__ uint32_t tiled_u8_bcast(uint32_t v, int src) {
    if constexpr (LPR == 64) return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), src));
    else return static_cast<uint32_t>(__shfl(static_cast<int>(v), src, LPR));
}

// ---- the row view ------------------------------------------------------------------------------------------------------------------------
// One workgroup (256 threads) per 32-row block `rb`. A ROW GROUP `g` of LPR lanes (16, 32 or a whole wave) owns RPG = 32 / (256 / LPR)
// output rows of the block, lane l on the columns cb .. cb + 3. The group walks the block's tiles once: lanes 0 .. RPG - 1 load the
// 16-byte tile rows of the group's rows (the next tile's while this one is decoded), every row's four words are broadcast, ANDed with
// the neighbour bitmap's words of the tile's k-quad (loaded one tile ahead) and decoded into that row's own queue, lists[ri]. A
// workgroup whose word of the row bitmap is zero takes an empty tile range without reading row_ptr; a masked-out row of a live block
// does not load its tile rows. Row ri is drained into red[ri] after the last tile and handed to done(ri), the kernel's epilogue, at once.
template <int LPR, class R, class Done>
__device__ __forceinline__ void tiled_u8_row_walk(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, uint64_t n_tiles, int n,
                                                  const uint8_t *Q, size_t ld, int cb, bool mine_cols, int (*lists)[TILED_U8_CAP],
                                                  const TiledNodes &nodes, int rb, int g, int l, R (&red)[LPR / 8], Done &&done) {
    constexpr int RPG = LPR / 8;
    TiledNodesWalk<true> nd;
    const int nq = step128(n);
    nd.start(nodes, rb, g * RPG + l);
    uint64_t t0 = 0, t1 = 0;   // an adjacency without tiles may come without row_ptr
    if (n_tiles != 0 && nd.block_live()) {
        t0 = static_cast<uint64_t>(row_ptr[rb]);
        t1 = static_cast<uint64_t>(row_ptr[rb + 1]);
        t1 = t1 < n_tiles ? t1 : n_tiles;
    }
    int cnt[RPG];
#pragma unroll
    for (int ri = 0; ri < RPG; ++ri) {
        cnt[ri] = 0;
        red[ri].reset();
    }
    const uint32_t *mine = tiles + (g * RPG + (l < RPG ? l : 0)) * 4;   // lane l < RPG: row g * RPG + l of every tile
    uint4 a = make_uint4(0, 0, 0, 0);
    int q = -1;
    if (t0 < t1) {
        q = kquad[t0];
        if (l < RPG && nd.row_live()) a = *reinterpret_cast<const uint4 *>(mine + t0 * 128);
        nd.load(nd.nb, q, nq);
    }
    for (uint64_t t = t0; t < t1; ++t) {
        uint4 an = make_uint4(0, 0, 0, 0);
        int qn = -1;
        if (t + 1 < t1) {
            qn = kquad[t + 1];
            if (l < RPG && nd.row_live()) an = *reinterpret_cast<const uint4 *>(mine + (t + 1) * 128);
            nd.load(nd.nbn, qn, nq);
        }
        if (static_cast<unsigned>(q) < static_cast<unsigned>(nq) && nd.tile_live()) {
            const uint32_t w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
            for (int ri = 0; ri < RPG; ++ri)
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    tiled_u8_decode(tiled_u8_bcast<LPR>(w[k], ri) & nd.word(k), q * 128 + k * 32, n, red[ri], lists[ri], cnt[ri], Q, ld, cb,
                                    mine_cols);
        }
        a = an;
        q = qn;
        nd.nb = nd.nbn;
    }
#pragma unroll
    for (int ri = 0; ri < RPG; ++ri) {
        red[ri].fold(lists[ri], cnt[ri], Q, ld, cb, mine_cols);
        done(ri);
    }
}

// ---- the column view ---------------------------------------------------------------------------------------------------------------------
// One workgroup (256 threads) per k-quad q (output rows 128 q .. 128 q + 127). The k-quad's column list is walked TS = 8 tiles a round,
// as in k_tiled_mm_f32_t: each half-wave loads one tile (its list entry two rounds, its words one round ahead), ANDs both bitmaps into
// the words and runs the 32 x 32 bit transpose; the column masks go to LDS as mk[tile column][staged tile], the tiles' row blocks to
// srb. A row group g of LPR lanes owns the output rows j = g, g + G, ..; a row with a mask in this round fetches its state from
// acc[j * LPR + l] and aux[j], decodes the staged tiles into `list`, reduces the addressed rows of Q and puts the state back (each word
// is read and written by one row group only). `r` brings what the reducer keeps outside its state; LDS starts as reset states.
template <int LPR, class R>
__device__ __forceinline__ void tiled_u8_col_walk(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles,
                                                  uint64_t n_tiles, int n, const uint8_t *Q, size_t ld, int cb, bool mine_cols,
                                                  const TiledNodes &nodes, int q, int g, int l, uint32_t *mk, int *srb, int *list,
                                                  typename R::Acc *acc, int *aux, R r) {
    constexpr int G = 256 / LPR, TS = TILED_T_TS;
    static_assert(TS == 8, "an output row reads its 8 masks of a round as two uint4");
    const int tid = threadIdx.x, nrb = (n + 31) / 32;
    r.reset();
    for (int j = g; j < 128; j += G) r.put(acc, aux, j * LPR + l, j);

    const int lane = tid & 31, s_own = tid >> 5;   // transposer role: half-wave s of the workgroup stages tile base + s
    uint64_t b0 = 0, t1 = 0;                       // an adjacency without tiles may come without col_ptr
    const uint4 rw = tiled_nodes_quad(nodes.row, q);   // the row bitmap's words of this k-quad
    if (n_tiles != 0 && (rw.x | rw.y | rw.z | rw.w) != 0) {
        b0 = static_cast<uint64_t>(col_ptr[q]);
        t1 = static_cast<uint64_t>(col_ptr[q + 1]);
        t1 = t1 < n_tiles ? t1 : n_tiles;
    }
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
            const uint32_t nb = nodes.nbr ? nodes.nbr[rb] : 0xffffffffu;   // rb < S32(n) <= S128(n) * 4
            if (nb) {   // a tile without a live neighbour is not read
                const uint4 r4 = *reinterpret_cast<const uint4 *>(tiles + t * 128 + (31 - lane) * 4);
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
            if (q * 128 + j >= n) break;
            const uint4 ma = *reinterpret_cast<const uint4 *>(mk + j * TS), mb = *reinterpret_cast<const uint4 *>(mk + j * TS + 4);
            const uint32_t m[TS] = {ma.x, ma.y, ma.z, ma.w, mb.x, mb.y, mb.z, mb.w};
            if (!(ma.x | ma.y | ma.z | ma.w | mb.x | mb.y | mb.z | mb.w)) continue;
            r.fetch(acc, aux, j * LPR + l, j);
            int cnt = 0;
#pragma unroll
            for (int st = 0; st < TS; ++st)
                if (m[st]) tiled_u8_decode(m[st], srb[st] * 32, n, r, list, cnt, Q, ld, cb, mine_cols);
            r.fold(list, cnt, Q, ld, cb, mine_cols);
            r.put(acc, aux, j * LPR + l, j);
        }
        __syncthreads();
    }
}

}  // namespace
