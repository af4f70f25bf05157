// tiled_codes_max_kernels.hip.h — part of libqgtc_hip.so (included by qgtc_tiled_codes_max.hip and qgtc_tiled_codes_max_t.hip, after
// common.hip.h and bitmm_popcount.hip.h): max and min aggregation on byte codes (include/qgtc_codes_max.h) - the
// element-wise extremum of the neighbours' rows of a uint8 code matrix on the tile-compressed adjacency, on both views, under node
// masks, stored as codes, as their dequantised float or as that float's codes under another row.
//
// The tile walk, the decode queue (TILED_U8_CAP ids in LDS, decoded MSB first), the load-ahead (TILED_U8_AHEAD rows in flight), the
// staging and bit transpose of the column view, the quantiser and the argument predicates are those of tiled_codes_kernels.hip.h, which
// this header includes. The reducer and its state are not:
//   - a lane owns four adjacent columns and keeps ONE packed dword per output row, never widened: the byte-wise maximum of two dwords is
//     taken on their even and odd bytes as two packed 16-bit maxima (v_pk_max_u16), the halves split once when a queue is drained and
//     joined once after it - a quarter of the sum walk's registers, and on the column view a quarter of its LDS, so that view too has the
//     64-lane class and chunks of 256 columns;
//   - min is max on complemented bytes: every loaded dword is XORed with `flip` (0, or 0xffffffff for min) and the finished dword is XORed
//     back, so the running identity is 0 either way, a lane that loads nothing contributes 0, and max / min is one uniform kernel
//     argument instead of a second set of instantiations;
//   - a maximum is idempotent: the load-ahead's surplus slots, which load the queue's last entry again, are reduced like any other -
//     no predicate per slot;
//   - there is no term count, only whether a row had a term at all: an extremum over nothing has no value, and the epilogue gives such a
//     row `empty` (codes), +0 (float) or the zero point (codes under another row).
#pragma once

#include "tiled_codes_kernels.hip.h"

namespace {

typedef unsigned short tiled_max_u16x2 __attribute__((ext_vector_type(2)));

// what a walk stores: the extremum codes as they are, their dequantised float, or that float re-quantised under the caller's row
constexpr int TILED_MAX_RAW = 0, TILED_MAX_FLOAT = 1, TILED_MAX_CODES = 2;

// the output of a walk as one kernel argument; a kernel reads the fields of its own form only
struct TiledMaxOut {
    void *p;             // RAW / CODES: code matrix [n, N], rows ld bytes apart; FLOAT: float32 [n, N], contiguous
    size_t ld;
    const float4 *oqp;   // CODES: the output's qparams row (scale, zero point, inverse scale, 0)
    float qmax;          // CODES: 2^out_bits - 1
    uint32_t empty;      // RAW: the code of a row without a term, in all four bytes
};

// s = bytewise max(s, Q[list[j]][cb .. cb + 3] ^ flip) over j < cnt. The loads of TILED_U8_AHEAD neighbours are issued together; past
// the end of the list the last entry is loaded again and reduced again, which changes nothing. `mine`: the lane's first column lies
// inside N, otherwise it loads nothing and keeps 0. The surplus bytes of a dword that straddles N are reduced too and dropped at the
// store. `list` lives in LDS and every lane of the row group wrote every entry itself.
__device__ __forceinline__ uint32_t tiled_max_rows(uint32_t s, const int *list, int cnt, const uint8_t *__restrict__ Q, size_t ld, int cb,
                                                   bool mine, uint32_t flip) {
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
    return __builtin_bit_cast(uint32_t, ev) | (__builtin_bit_cast(uint32_t, od) << 8);
}

// the set bits of `m`, MSB first, as neighbour ids base + (leading zeros), queued in `list`; ids from n up are dropped (a foreign tile
// must not make the kernel read past Q). `had` records that the row queued a term. A full queue is reduced at once.
__device__ __forceinline__ void tiled_max_decode(uint32_t m, int base, int n, uint32_t &s, int *list, int &cnt, bool &had,
                                                 const uint8_t *__restrict__ Q, size_t ld, int cb, bool mine, uint32_t flip) {
    while (m) {
        const int b = __builtin_clz(m);
        m &= ~(0x80000000u >> b);
        const int v = base + b;
        if (v < n) {
            list[cnt++] = v;
            had = true;
            if (cnt == TILED_U8_CAP) {
                s = tiled_max_rows(s, list, cnt, Q, ld, cb, mine, flip);
                cnt = 0;
            }
        }
    }
}

// the epilogue of one output row's four columns (one dword of the row): `s` the running maximum in the flipped domain
template <int OUT>
__device__ __forceinline__ void tiled_max_store(uint32_t s, bool had, int row, int cb, int N, const float4 *__restrict__ qp, uint32_t flip,
                                                const TiledMaxOut &out) {
    if (cb >= N) return;
    const uint32_t m = s ^ flip;   // the extremum codes, column cb + k at byte k
    if constexpr (OUT == TILED_MAX_RAW) {
        const uint32_t keep = cb + 4 <= N ? 0xffffffffu : (1u << (8 * (N - cb))) - 1u;   // bytes N .. PAD4(N) - 1 are written 0
        *reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(out.p) + static_cast<uint64_t>(row) * out.ld + cb) = (had ? m : out.empty) & keep;
    } else {
        const float4 g = qp[0];
        const int z = static_cast<int>(g.y);
        float y[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            y[k] = had ? __fmul_rn(static_cast<float>(static_cast<int>((m >> (8 * k)) & 0xffu) - z), g.x) : 0.0f;
        if constexpr (OUT == TILED_MAX_FLOAT) {
            float *o = static_cast<float *>(out.p) + static_cast<uint64_t>(row) * N;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (cb + k < N) o[cb + k] = y[k];
        } else {
            const float4 og = out.oqp[0];
            uint32_t word = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) word |= (cb + k < N ? codes_quant(y[k], og.z, og.y, out.qmax) : 0u) << (8 * k);
            *reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(out.p) + static_cast<uint64_t>(row) * out.ld + cb) = word;
        }
    }
}

// ---- the row view: out = max over A_tiled's rows ----------------------------------------------------------------------------------------
// The split of k_tiled_mm_u8: one workgroup (256 threads) per 32-row block and chunk of 4 LPR output columns, a row group of LPR lanes on
// RPG = 32 / (256 / LPR) rows, lanes 0 .. RPG - 1 loading the group's 16-byte tile rows one tile ahead, every row's four words broadcast,
// ANDed with the neighbour bitmap's words and decoded into that row's own queue. Per row a lane holds one dword, one queue length and one
// flag bit.
template <int LPR, int OUT>
__global__ __launch_bounds__(256) void k_tiled_max_u8(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ kquad,
                                                      const uint32_t *__restrict__ tiles, uint64_t n_tiles, int n,
                                                      const uint8_t *__restrict__ Q, size_t ld, int N, const float4 *__restrict__ qp,
                                                      uint32_t flip, TiledMaxOut out, TiledNodes nodes) {
    constexpr int G = 256 / LPR, RPG = 32 / G;   // row groups per workgroup, rows per group
    TiledNodesWalk<true> nd;
    __shared__ int lists[G][RPG][TILED_U8_CAP];
    const int rb = blockIdx.x, tid = threadIdx.x;
    const int g = LPR == 64 ? __builtin_amdgcn_readfirstlane(tid / LPR) : tid / LPR;
    const int l = tid % LPR, cb = blockIdx.y * (LPR * 4) + l * 4;
    const bool mine_cols = cb < N;
    const int nq = step128(n);
    nd.start(nodes, rb, g * RPG + l);

    uint64_t t0 = 0, t1 = 0;   // an adjacency without tiles may come without row_ptr
    if (n_tiles != 0 && nd.block_live()) {
        t0 = static_cast<uint64_t>(row_ptr[rb]);
        t1 = static_cast<uint64_t>(row_ptr[rb + 1]);
        t1 = t1 < n_tiles ? t1 : n_tiles;
    }
    uint32_t s[RPG];
    int cnt[RPG];
    bool had[RPG];
#pragma unroll
    for (int ri = 0; ri < RPG; ++ri) {
        s[ri] = 0;
        cnt[ri] = 0;
        had[ri] = false;
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
                    tiled_max_decode(tiled_u8_bcast<LPR>(w[k], ri) & nd.word(k), q * 128 + k * 32, n, s[ri], lists[g][ri], cnt[ri], had[ri], Q,
                                     ld, cb, mine_cols, flip);
        }
        a = an;
        q = qn;
        nd.nb = nd.nbn;
    }
#pragma unroll
    for (int ri = 0; ri < RPG; ++ri) {
        s[ri] = tiled_max_rows(s[ri], lists[g][ri], cnt[ri], Q, ld, cb, mine_cols, flip);
        const int row = rb * 32 + g * RPG + ri;
        if (row < n) tiled_max_store<OUT>(s[ri], had[ri], row, cb, N, qp, flip, out);
    }
}

// ---- the column view: out = max over A_tiled^T's rows -----------------------------------------------------------------------------------
// The rounds of k_tiled_mm_u8_t: one workgroup per k-quad q (output rows 128 q .. 128 q + 127) and chunk of 4 LPR columns, TS = 8 tiles
// a round staged and bit-transposed by the half-waves, the column masks in LDS as [tile column][staged tile]. Between rounds the state
// of the 128 x 4 LPR outputs is ONE dword a lane and output row (128 LPR 4 bytes: 32 KiB at 64 lanes) and a flag word a row; each word is
// read and written by the lanes of one row group only, and every lane of the group writes the flag (the same value to the same address).
template <int LPR, int OUT>
__global__ __launch_bounds__(256) void k_tiled_max_u8_t(const int64_t *__restrict__ col_ptr, const int64_t *__restrict__ col_tile,
                                                        const int32_t *__restrict__ col_rb, const uint32_t *__restrict__ tiles,
                                                        uint64_t n_tiles, int n, const uint8_t *__restrict__ Q, size_t ld, int N,
                                                        const float4 *__restrict__ qp, uint32_t flip, TiledMaxOut out, TiledNodes nodes) {
    constexpr int G = 256 / LPR, TS = TILED_T_TS;
    static_assert(TS == 8, "an output row reads its 8 masks of a round as two uint4");
    __shared__ __attribute__((aligned(16))) uint32_t mk[128 * TS];   // [tile column][staged tile]
    __shared__ int srb[TS];
    __shared__ uint32_t acc[128 * LPR];                              // [output row][lane]: four columns' running maximum
    __shared__ int any[128];                                         // whether an output row had a term
    __shared__ int lists[G][TILED_U8_CAP];
    const int q = blockIdx.x, tid = threadIdx.x;
    const int g = LPR == 64 ? __builtin_amdgcn_readfirstlane(tid / LPR) : tid / LPR;
    const int l = tid % LPR, cb = blockIdx.y * (LPR * 4) + l * 4;
    const bool mine_cols = cb < N;
    const int nrb = (n + 31) / 32;
    int *list = lists[g];
    for (int j = g; j < 128; j += G) {
        acc[j * LPR + l] = 0;
        any[j] = 0;
    }

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
                const uint4 r = *reinterpret_cast<const uint4 *>(tiles + t * 128 + (31 - lane) * 4);
                const uint32_t on = (nb >> lane) & 1u ? 0xffffffffu : 0u;   // lane holds tile row 31 - lane: bit `lane` of the word
                return make_uint4(r.x & rw.x & on, r.y & rw.y & on, r.z & rw.z & on, r.w & rw.w & on);
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
            uint32_t s = acc[j * LPR + l];
            int cnt = 0;
            bool had = any[j] != 0;
#pragma unroll
            for (int st = 0; st < TS; ++st)
                if (m[st]) tiled_max_decode(m[st], srb[st] * 32, n, s, list, cnt, had, Q, ld, cb, mine_cols, flip);
            acc[j * LPR + l] = tiled_max_rows(s, list, cnt, Q, ld, cb, mine_cols, flip);
            any[j] = had;
        }
        __syncthreads();
    }

    for (int j = g; j < 128; j += G) {
        const int row = q * 128 + j;
        if (row >= n) break;
        tiled_max_store<OUT>(acc[j * LPR + l], any[j] != 0, row, cb, N, qp, flip, out);
    }
}

// ---- the host side: lanes per output row by N, the same classes on both views ----------------------------------------------------------
// N up to 64: 16 lanes; up to 128: 32 lanes; beyond: a whole wave and chunks of 256 columns (grid.y)
template <int OUT>
int tiled_max_launch(const TiledRowIndex &ix, const uint32_t *tiles, int64_t n_tiles, int n, const uint8_t *Q, size_t ld, int N,
                     const float *qparams, uint32_t flip, const TiledMaxOut &out, const TiledNodes &nodes, hipStream_t st) {
    tiled_u8_width_switch(N, 64, [&](auto lpr) {
        constexpr int LPR = decltype(lpr)::value;
        hipLaunchKernelGGL((k_tiled_max_u8<LPR, OUT>), dim3((n + 31) / 32, (N + LPR * 4 - 1) / (LPR * 4)), dim3(256), 0, st, ix.row_ptr,
                           ix.kquad, tiles, static_cast<uint64_t>(n_tiles), n, Q, ld, N, reinterpret_cast<const float4 *>(qparams), flip, out,
                           nodes);
    });
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

template <int OUT>
int tiled_max_launch(const TiledColIndex &ix, const uint32_t *tiles, int64_t n_tiles, int n, const uint8_t *Q, size_t ld, int N,
                     const float *qparams, uint32_t flip, const TiledMaxOut &out, const TiledNodes &nodes, hipStream_t st) {
    tiled_u8_width_switch(N, 64, [&](auto lpr) {
        constexpr int LPR = decltype(lpr)::value;
        hipLaunchKernelGGL((k_tiled_max_u8_t<LPR, OUT>), dim3(step128(n), (N + LPR * 4 - 1) / (LPR * 4)), dim3(256), 0, st, ix.col_ptr,
                           ix.col_tile, ix.col_rb, tiles, static_cast<uint64_t>(n_tiles), n, Q, ld, N,
                           reinterpret_cast<const float4 *>(qparams), flip, out, nodes);
    });
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

// ---- the entries' bodies, either view: invalid, then misaligned, then short, then the launch -----------------------------------------
template <class Index>
int tiled_max_raw_entry(const Index &ix, const uint32_t *tiles, int64_t n_tiles, int n, const uint8_t *Q, size_t ld, size_t q_bytes, int N,
                        int is_min, int empty_code, uint8_t *out, size_t ldo, size_t out_bytes, const uint32_t *row_mask,
                        const uint32_t *nbr_mask, size_t mask_words, void *stream) {
    if (!Q || !out || N < 1 || empty_code < 0 || empty_code > 255 || tiled_adj_malformed(ix.ok(), tiles, n_tiles, n)) return QGTC_EINVAL;
    if (tiled_adj_misaligned(tiles) || codes_matrix_misaligned(Q, ld, N) || codes_matrix_misaligned(out, ldo, N) || !aligned16(row_mask) ||
        !aligned16(nbr_mask))
        return QGTC_EALIGN;
    if (q_bytes < codes_matrix_bytes(n, N, ld) || out_bytes < codes_matrix_bytes(n, N, ldo)) return QGTC_ESIZE;
    if ((row_mask || nbr_mask) && mask_words < static_cast<size_t>(step128(n)) * 4) return QGTC_ESIZE;
    const TiledMaxOut dst{out, ldo, nullptr, 0.0f, static_cast<uint32_t>(empty_code) * 0x01010101u};
    return tiled_max_launch<TILED_MAX_RAW>(ix, tiles, n_tiles, n, Q, ld, N, nullptr, is_min ? 0xffffffffu : 0u, dst,
                                           TiledNodes{row_mask, nbr_mask}, static_cast<hipStream_t>(stream));
}

template <class Index>
int tiled_max_affine_entry(const Index &ix, const uint32_t *tiles, int64_t n_tiles, int n, const uint8_t *Q, size_t ld, size_t q_bytes, int N,
                           const float *qparams, int is_min, float *out, size_t out_elems, uint8_t *outq, size_t ldo, size_t outq_bytes,
                           const float *out_qp, int out_bits, const uint32_t *row_mask, const uint32_t *nbr_mask, size_t mask_words,
                           void *stream) {
    if (!Q || !qparams || N < 1 || (out != nullptr) == (outq != nullptr) || (outq && (!out_qp || out_bits < 1 || out_bits > 8)) ||
        tiled_adj_malformed(ix.ok(), tiles, n_tiles, n))
        return QGTC_EINVAL;
    if (tiled_adj_misaligned(tiles) || codes_matrix_misaligned(Q, ld, N) || !aligned16(qparams) || !codes_aligned4(out) ||
        (outq && (codes_matrix_misaligned(outq, ldo, N) || !aligned16(out_qp))) || !aligned16(row_mask) || !aligned16(nbr_mask))
        return QGTC_EALIGN;
    if (q_bytes < codes_matrix_bytes(n, N, ld) || (out && out_elems < static_cast<size_t>(n) * static_cast<size_t>(N)) ||
        (outq && outq_bytes < codes_matrix_bytes(n, N, ldo)))
        return QGTC_ESIZE;
    if ((row_mask || nbr_mask) && mask_words < static_cast<size_t>(step128(n)) * 4) return QGTC_ESIZE;
    const uint32_t flip = is_min ? 0xffffffffu : 0u;
    const TiledNodes nodes{row_mask, nbr_mask};
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (out) return tiled_max_launch<TILED_MAX_FLOAT>(ix, tiles, n_tiles, n, Q, ld, N, qparams, flip, TiledMaxOut{out, 0, nullptr, 0.0f, 0u}, nodes, st);
    const TiledMaxOut dst{outq, ldo, reinterpret_cast<const float4 *>(out_qp), static_cast<float>((1 << out_bits) - 1), 0u};
    return tiled_max_launch<TILED_MAX_CODES>(ix, tiles, n_tiles, n, Q, ld, N, qparams, flip, dst, nodes, st);
}

}  // namespace
