// tiled_codes_kernels.hip.h — part of libqgtc_hip.so (included by qgtc_tiled_codes.hip and qgtc_tiled_codes_t.hip, after common.hip.h and
// bitmm_popcount.hip.h): the byte-code route of affine quantisation (include/qgtc_codes.h) - the quantiser to
// one byte a code, and the neighbour sum of a uint8 code matrix on the tile-compressed adjacency, on both views, under node masks, with
// the dequantising epilogue of qgtc_affine_dequant in the same launch.
// The family's shared tile walks are tiled_codes_walk.hip.h's; the walk is described there. k_tiled_mm_u8 and k_tiled_mm_u8_t below
// keep their own copy of it, with their own adder and decoder: on the shared walk the 16-lane float-output sum ran 2 to 4 % longer
// (profiles/codes_walk/README.md). Here besides: the quantiser, the sum's three output forms, and what the
// whole byte-code family shares on the host - the width rule, the one launcher per view and the argument predicates.
#pragma once

#include "tiled_codes_walk.hip.h"

namespace {

// ---- the quantiser to bytes -----------------------------------------------------------------------------------------------------------
// aquant of affine_kernels.hip.h, to the letter: one multiply, one v_rndne, one add, a clamp, and the select that sends a NaN to the zero
// point. __fmul_rn / __fadd_rn: hipcc contracts a * b + c into an FMA otherwise.
__device__ __forceinline__ uint32_t codes_quant(float x, float inv, float zp, float qmax) {
    const float y = __fmul_rn(x, inv);
    const float c = fminf(fmaxf(__fadd_rn(rintf(y), zp), 0.0f), qmax);
    return static_cast<uint32_t>(y != y ? zp : c);
}

// One thread per output dword (columns 4 j .. 4 j + 3 of a row), grid-stride: VEC (W % 4 == 0 and a 16-byte aligned x) reads a float4,
// otherwise up to four floats; a column past W gets the code 0 (bytes W .. PAD4(W) - 1 are written 0). Code c of the dword sits at byte c:
// bits 8 (c & 3) .. on this little-endian device.
template <bool VEC, bool PERCOL>
__global__ __launch_bounds__(256) void k_affine_codes(const float *__restrict__ x, int H, int W, float qmax, const float4 *__restrict__ qp,
                                                      uint8_t *__restrict__ out, size_t ld, unsigned nthreads) {
    const uint32_t W4 = (static_cast<uint32_t>(W) + 3u) >> 2;
    const unsigned long long total = static_cast<unsigned long long>(H) * W4;
    const bool small = total < (1ull << 32);
    const float4 g0 = qp[0];
    for (unsigned long long idx = blockIdx.x * 256ull + threadIdx.x; idx < total; idx += nthreads) {
        uint32_t r, j;
        if (small) {
            const uint32_t i32 = static_cast<uint32_t>(idx);
            r = i32 / W4;
            j = i32 - r * W4;
        } else {
            r = static_cast<uint32_t>(idx / W4);
            j = static_cast<uint32_t>(idx % W4);
        }
        const int c = static_cast<int>(j * 4u);
        const float *row = x + static_cast<size_t>(r) * W + c;
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if constexpr (VEC) {
            const float4 f = *reinterpret_cast<const float4 *>(row);
            v[0] = f.x, v[1] = f.y, v[2] = f.z, v[3] = f.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (c + k < W) v[k] = row[k];
        }
        uint32_t word = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float zp = g0.y, inv = g0.z;
            if constexpr (PERCOL) {
                const float4 g = qp[c + k < W ? c + k : 0];
                zp = g.y, inv = g.z;
            }
            const uint32_t q = c + k < W ? codes_quant(v[k], inv, zp, qmax) : 0u;
            word |= q << (8 * k);
        }
        *reinterpret_cast<uint32_t *>(out + static_cast<size_t>(r) * ld + c) = word;
    }
}

// tiled_u8_decode of tiled_codes_walk.hip.h on the two sum kernels' own state: ids counted in `terms`, a full queue added at once
__device__ __forceinline__ void tiled_u8_decode(uint32_t m, int base, int n, int (&s)[4], int *list, int &cnt, int &terms,
                                                const uint8_t *__restrict__ Q, size_t ld, int cb, bool mine) {
    while (m) {
        const int b = __builtin_clz(m);
        m &= ~(0x80000000u >> b);
        const int v = base + b;
        if (v < n) {
            list[cnt++] = v;
            ++terms;
            if (cnt == TILED_U8_CAP) {
                tiled_u8_add_rows(s, list, cnt, Q, ld, cb, mine);
                cnt = 0;
            }
        }
    }
}

// the epilogue of one output row's four columns: the int sums, or (AFFINE) t = acc - z * terms in 64 bits, one conversion, one multiply by
// the scale and one by row_scale[row] when given - separate IEEE operations, as k_affine_dequant makes them
__device__ __forceinline__ float tiled_u8_dequant(int acc, int terms, long long z, float scale, bool scaled, float rs) {
#pragma clang fp contract(off)
    const long long t = static_cast<long long>(acc) - z * static_cast<long long>(terms);
    float y = static_cast<float>(t) * scale;
    if (scaled) y = y * rs;
    return y;
}

// what a walk stores (the AFFINE switch of everything below): the int32 sums, their dequantised float, or that float re-quantised to one
// byte a code under the caller's fixed output row (include/qgtc_chain.h)
constexpr int TILED_U8_SUMS = 0, TILED_U8_FLOAT = 1, TILED_U8_CODES = 2;

// the output of a walk as a kernel argument: a plain pointer for sums and floats, the code matrix and its row for codes
struct TiledU8Codes {
    uint8_t *q;         // code matrix [n, N], rows ld bytes apart
    size_t ld;
    const float4 *qp;   // its qparams row (scale, zero point, inverse scale, 0), per tensor
    float qmax;
};
template <int AFFINE>
struct TiledU8Out {
    using type = void *__restrict__;
};
template <>
struct TiledU8Out<TILED_U8_CODES> {
    using type = TiledU8Codes;
};

template <int AFFINE>
__device__ __forceinline__ void tiled_u8_store(const int (&s)[4], int terms, int row, int cb, int N, const float4 *__restrict__ qp,
                                               const float *__restrict__ row_scale, typename TiledU8Out<AFFINE>::type out) {
    if constexpr (AFFINE == TILED_U8_CODES) {
        // the lane's four adjacent columns are one aligned dword of the row: four quantisers, one store; a column past N is the byte 0
        const float4 g = qp[0], og = out.qp[0];
        const long long z = static_cast<long long>(g.y);
        const float rs = row_scale ? row_scale[row] : 1.0f;
        uint32_t word = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t c = codes_quant(tiled_u8_dequant(s[k], terms, z, g.x, row_scale != nullptr, rs), og.z, og.y, out.qmax);
            word |= (cb + k < N ? c : 0u) << (8 * k);
        }
        if (cb < N) *reinterpret_cast<uint32_t *>(out.q + static_cast<uint64_t>(row) * out.ld + cb) = word;
    } else if constexpr (AFFINE == TILED_U8_FLOAT) {
        const float4 g = qp[0];
        const long long z = static_cast<long long>(g.y);
        const float rs = row_scale ? row_scale[row] : 1.0f;
        float *o = static_cast<float *>(out) + static_cast<uint64_t>(row) * N;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (cb + k < N) o[cb + k] = tiled_u8_dequant(s[k], terms, z, g.x, row_scale != nullptr, rs);
    } else {
        int *o = static_cast<int *>(out) + static_cast<uint64_t>(row) * N;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (cb + k < N) o[cb + k] = s[k];
    }
}

// ---- the row view: out = A_tiled . Q --------------------------------------------------------------------------------------------------
// The row walk of tiled_codes_walk.hip.h (tiled_u8_row_walk describes it), written out here for the sum, per chunk of 4 LPR output
// columns (grid.y). Every row of the block is stored once, through the epilogue.
template <int LPR, int AFFINE>
__global__ __launch_bounds__(256) void k_tiled_mm_u8(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ kquad,
                                                     const uint32_t *__restrict__ tiles, uint64_t n_tiles, int n,
                                                     const uint8_t *__restrict__ Q, size_t ld, int N, const float4 *__restrict__ qp,
                                                     const float *__restrict__ row_scale, typename TiledU8Out<AFFINE>::type out, TiledNodes nodes) {
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
    int s[RPG][4], cnt[RPG], terms[RPG];
#pragma unroll
    for (int ri = 0; ri < RPG; ++ri) {
        cnt[ri] = terms[ri] = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) s[ri][k] = 0;
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
                    tiled_u8_decode(tiled_u8_bcast<LPR>(w[k], ri) & nd.word(k), q * 128 + k * 32, n, s[ri], lists[g][ri], cnt[ri], terms[ri], Q,
                                    ld, cb, mine_cols);
        }
        a = an;
        q = qn;
        nd.nb = nd.nbn;
    }
#pragma unroll
    for (int ri = 0; ri < RPG; ++ri) {
        tiled_u8_add_rows(s[ri], lists[g][ri], cnt[ri], Q, ld, cb, mine_cols);
        const int row = rb * 32 + g * RPG + ri;
        if (row < n) tiled_u8_store<AFFINE>(s[ri], terms[ri], row, cb, N, qp, row_scale, out);
    }
}

// ---- the column view: out = A_tiled^T . Q ---------------------------------------------------------------------------------------------
// The column walk of tiled_codes_walk.hip.h (tiled_u8_col_walk describes it), written out here for the sum: the running sums of the
// 128 x 4 LPR outputs (int32, one int4 a lane) and the 128 term counters beside them live in LDS between rounds. A k-quad whose four
// row-bitmap words are zero walks nothing and stores its rows through the epilogue with acc = cnt = 0.
template <int LPR, int AFFINE>
__global__ __launch_bounds__(256) void k_tiled_mm_u8_t(const int64_t *__restrict__ col_ptr, const int64_t *__restrict__ col_tile,
                                                       const int32_t *__restrict__ col_rb, const uint32_t *__restrict__ tiles,
                                                       uint64_t n_tiles, int n, const uint8_t *__restrict__ Q, size_t ld, int N,
                                                       const float4 *__restrict__ qp, const float *__restrict__ row_scale,
                                                       typename TiledU8Out<AFFINE>::type out, TiledNodes nodes) {
    constexpr int G = 256 / LPR, TS = TILED_T_TS;
    static_assert(TS == 8, "an output row reads its 8 masks of a round as two uint4");
    __shared__ __attribute__((aligned(16))) uint32_t mk[128 * TS];   // [tile column][staged tile]
    __shared__ int srb[TS];
    __shared__ __attribute__((aligned(16))) int acc[128 * LPR * 4];  // [output row][lane][4 columns]
    __shared__ int tot[128];                                         // terms added into every output row
    __shared__ int lists[G][TILED_U8_CAP];
    const int q = blockIdx.x, tid = threadIdx.x;
    const int g = LPR == 64 ? __builtin_amdgcn_readfirstlane(tid / LPR) : tid / LPR;
    const int l = tid % LPR, cb = blockIdx.y * (LPR * 4) + l * 4;
    const bool mine_cols = cb < N;
    const int nrb = (n + 31) / 32;
    int *list = lists[g];
    int4 *acc4 = reinterpret_cast<int4 *>(acc);
    for (int j = g; j < 128; j += G) {
        acc4[j * LPR + l] = make_int4(0, 0, 0, 0);
        tot[j] = 0;
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
            const int4 s4 = acc4[j * LPR + l];
            int s[4] = {s4.x, s4.y, s4.z, s4.w};
            int cnt = 0, terms = tot[j];
#pragma unroll
            for (int st = 0; st < TS; ++st)
                if (m[st]) tiled_u8_decode(m[st], srb[st] * 32, n, s, list, cnt, terms, Q, ld, cb, mine_cols);
            tiled_u8_add_rows(s, list, cnt, Q, ld, cb, mine_cols);
            acc4[j * LPR + l] = make_int4(s[0], s[1], s[2], s[3]);
            tot[j] = terms;
        }
        __syncthreads();
    }

    for (int j = g; j < 128; j += G) {
        const int row = q * 128 + j;
        if (row >= n) break;
        const int4 s4 = acc4[j * LPR + l];
        const int s[4] = {s4.x, s4.y, s4.z, s4.w};
        tiled_u8_store<AFFINE>(s, tot[j], row, cb, N, qp, row_scale, out);
    }
}

// ---- the host side of the family: lanes per output row by N, one launcher per view -------------------------------------------------------
// N up to 64: 16 lanes; up to 128: 32 lanes; beyond: a whole wave and chunks of 256 columns (grid.y), if the view has that class
template <class F>
void tiled_u8_width_switch(int N, int widest, F &&launch) {
    const int lanes = N <= 64 ? 16 : (N <= 128 || widest == 32 ? 32 : 64);
    switch (lanes) {
        case 16: launch(tiled_int<16>{}); break;
        case 32: launch(tiled_int<32>{}); break;
        default: launch(tiled_int<64>{}); break;
    }
}

// what every entry of the family is given: the adjacency's tiles, the code matrix Q [n, N] and the node masks
struct TiledU8In {
    const uint32_t *tiles;
    int64_t n_tiles;
    int n;
    const uint8_t *Q;
    size_t ld, q_bytes;
    int N;
    const uint32_t *row_mask, *nbr_mask;
    size_t mask_words;
};

// A kernel family as the launchers take it: its kernels and the column view's widest class (the sum's LDS is 128 KiB at 64 lanes: 32).
template <int AFFINE>
struct TiledU8SumKernels {
    static constexpr int COL_WIDEST = 32;
    template <int LPR> static auto row() { return k_tiled_mm_u8<LPR, AFFINE>; }
    template <int LPR> static auto col() { return k_tiled_mm_u8_t<LPR, AFFINE>; }
};

// `tail`: the family's kernel arguments between N and the node masks, in the kernels' order and types - for TiledU8SumKernels
// (const float4 *qp, const float *row_scale, TiledU8Out<AFFINE>::type out). A unit instantiates the kernels it passes and no others.
template <class F, class... Tail>
int tiled_u8_launch(const TiledRowIndex &ix, const TiledU8In &a, void *stream, Tail... tail) {
    const TiledNodes nodes{a.row_mask, a.nbr_mask};
    tiled_u8_width_switch(a.N, 64, [&](auto lpr) {
        constexpr int LPR = decltype(lpr)::value;
        hipLaunchKernelGGL((F::template row<LPR>()), dim3((a.n + 31) / 32, (a.N + LPR * 4 - 1) / (LPR * 4)), dim3(256), 0,
                           static_cast<hipStream_t>(stream), ix.row_ptr, ix.kquad, a.tiles, static_cast<uint64_t>(a.n_tiles), a.n, a.Q, a.ld,
                           a.N, tail..., nodes);
    });
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

template <class F, class... Tail>
int tiled_u8_launch(const TiledColIndex &ix, const TiledU8In &a, void *stream, Tail... tail) {
    const TiledNodes nodes{a.row_mask, a.nbr_mask};
    tiled_u8_width_switch(a.N, F::COL_WIDEST, [&](auto lpr) {
        constexpr int LPR = decltype(lpr)::value;
        if constexpr (LPR <= F::COL_WIDEST)
            hipLaunchKernelGGL((F::template col<LPR>()), dim3(step128(a.n), (a.N + LPR * 4 - 1) / (LPR * 4)), dim3(256), 0,
                               static_cast<hipStream_t>(stream), ix.col_ptr, ix.col_tile, ix.col_rb, a.tiles, static_cast<uint64_t>(a.n_tiles),
                               a.n, a.Q, a.ld, a.N, tail..., nodes);
    });
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

// ---- the argument checks, made before any device work: invalid, then misaligned, then short ------------------------------------------
// One predicate per error class and part of the argument list, so that an entry ORs its own clauses with them class by class and still
// reports every invalid argument before any misaligned one and every misaligned one before any short one.
inline bool codes_aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
inline size_t codes_pad4(int W) { return (static_cast<size_t>(W) + 3u) & ~static_cast<size_t>(3); }
// the three rules of a code matrix [H, W]
inline bool codes_matrix_misaligned(const void *p, size_t ld, int W) {
    return !codes_aligned4(p) || ld < static_cast<size_t>(W) || (ld & 3u) != 0;
}
inline size_t codes_matrix_bytes(int H, int W, size_t ld) { return static_cast<size_t>(H - 1) * ld + codes_pad4(W); }

// what every entry shares: the graph, the code matrix, the masks
template <class Index>
bool tiled_u8_invalid(const Index &ix, const TiledU8In &a) {
    return !a.Q || a.N < 1 || tiled_adj_malformed(ix.ok(), a.tiles, a.n_tiles, a.n);
}
inline bool tiled_u8_misaligned(const TiledU8In &a) {
    return tiled_adj_misaligned(a.tiles) || codes_matrix_misaligned(a.Q, a.ld, a.N) || !aligned16(a.row_mask) || !aligned16(a.nbr_mask);
}
inline bool tiled_u8_short(const TiledU8In &a) {
    return a.q_bytes < codes_matrix_bytes(a.n, a.N, a.ld) || ((a.row_mask || a.nbr_mask) && a.mask_words < static_cast<size_t>(step128(a.n)) * 4);
}

// the destination of the static chain's entries: float32 [H, W] at `out` or codes [H, W] at `outq` under the row (out_qp, out_bits), not both
struct CodesDest {
    float *out;
    size_t out_elems;
    uint8_t *outq;
    size_t ldo, outq_bytes;
    const float *out_qp;
    int out_bits;
    const float4 *qp() const { return reinterpret_cast<const float4 *>(out_qp); }
    float qmax() const { return outq ? static_cast<float>((1 << out_bits) - 1) : 0.0f; }
};
inline bool codes_dest_invalid(const CodesDest &d) {
    return (d.out != nullptr) == (d.outq != nullptr) || (d.outq && (!d.out_qp || d.out_bits < 1 || d.out_bits > 8));
}
inline bool codes_dest_misaligned(const CodesDest &d, int W) {
    return !codes_aligned4(d.out) || (d.outq && (codes_matrix_misaligned(d.outq, d.ldo, W) || !aligned16(d.out_qp)));
}
inline bool codes_dest_short(const CodesDest &d, int H, int W) {
    return (d.out && d.out_elems < static_cast<size_t>(H) * static_cast<size_t>(W)) || (d.outq && d.outq_bytes < codes_matrix_bytes(H, W, d.ldo));
}

// either view; AFFINE wants qparams (16-byte aligned) and takes an optional row_scale
template <int AFFINE, class Index>
int tiled_u8_entry(const Index &ix, const TiledU8In &a, const float *qparams, const float *row_scale, void *out, size_t out_elems,
                   void *stream) {
    if (tiled_u8_invalid(ix, a) || !out || (AFFINE && !qparams)) return QGTC_EINVAL;
    if (tiled_u8_misaligned(a) || !codes_aligned4(out) || !aligned16(qparams) || !codes_aligned4(row_scale)) return QGTC_EALIGN;
    if (tiled_u8_short(a) || out_elems < static_cast<size_t>(a.n) * static_cast<size_t>(a.N)) return QGTC_ESIZE;
    return tiled_u8_launch<TiledU8SumKernels<AFFINE>>(ix, a, stream, reinterpret_cast<const float4 *>(qparams), row_scale, out);
}

// either view with the code output of include/qgtc_chain.h: d.outq a code matrix [n, N] under (d.out_qp, d.out_bits), d.out null
template <class Index>
int tiled_u8_requant_entry(const Index &ix, const TiledU8In &a, const float *qparams, const float *row_scale, const CodesDest &d,
                           void *stream) {
    if (tiled_u8_invalid(ix, a) || codes_dest_invalid(d) || !qparams) return QGTC_EINVAL;
    if (tiled_u8_misaligned(a) || codes_dest_misaligned(d, a.N) || !aligned16(qparams) || !codes_aligned4(row_scale)) return QGTC_EALIGN;
    if (tiled_u8_short(a) || codes_dest_short(d, a.n, a.N)) return QGTC_ESIZE;
    return tiled_u8_launch<TiledU8SumKernels<TILED_U8_CODES>>(ix, a, stream, reinterpret_cast<const float4 *>(qparams), row_scale,
                                                              TiledU8Codes{d.outq, d.ldo, d.qp(), d.qmax()});
}

}  // namespace
