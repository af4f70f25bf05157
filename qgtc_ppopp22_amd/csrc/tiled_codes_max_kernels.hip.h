// tiled_codes_max_kernels.hip.h — part of libqgtc_hip.so (included by qgtc_tiled_codes_max.hip and qgtc_tiled_codes_max_t.hip, after
// common.hip.h and bitmm_popcount.hip.h): max and min aggregation on byte codes (include/qgtc_codes_max.h) - the
// element-wise extremum of the neighbours' rows of a uint8 code matrix on the tile-compressed adjacency, on both views, under node
// masks, stored as codes, as their dequantised float or as that float's codes under another row.
//
// The tile walks with the extremum reducer (TiledU8Extremum) are tiled_codes_walk.hip.h's; the quantiser, the launchers and the argument
// predicates are those of tiled_codes_kernels.hip.h, which this header includes. Here: the three output forms, the two kernels and the
// entries' bodies. The reducer keeps one dword a lane and output row - a quarter of the sum's registers, and on the column view a
// quarter of its LDS, so that view too has the 64-lane class and chunks of 256 columns. Max / min is one uniform kernel argument
// (`flip`) instead of a second set of instantiations. A row without a term gets `empty` (codes), +0 (float) or the zero point (codes
// under another row) from the epilogue.
#pragma once

#include "tiled_codes_kernels.hip.h"

namespace {

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
// tiled_u8_row_walk with the extremum, per chunk of 4 LPR output columns: per row a lane holds one dword, one queue length and one flag.
template <int LPR, int OUT>
__global__ __launch_bounds__(256) void k_tiled_max_u8(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ kquad,
                                                      const uint32_t *__restrict__ tiles, uint64_t n_tiles, int n,
                                                      const uint8_t *__restrict__ Q, size_t ld, int N, const float4 *__restrict__ qp,
                                                      uint32_t flip, TiledMaxOut out, TiledNodes nodes) {
    constexpr int G = 256 / LPR, RPG = 32 / G;   // row groups per workgroup, rows per group
    __shared__ int lists[G][RPG][TILED_U8_CAP];
    const int rb = blockIdx.x, tid = threadIdx.x;
    const int g = LPR == 64 ? __builtin_amdgcn_readfirstlane(tid / LPR) : tid / LPR;
    const int l = tid % LPR, cb = blockIdx.y * (LPR * 4) + l * 4;
    const bool mine_cols = cb < N;
    TiledU8Extremum red[RPG];
#pragma unroll
    for (int ri = 0; ri < RPG; ++ri) red[ri].flip = flip;
    tiled_u8_row_walk<LPR>(row_ptr, kquad, tiles, n_tiles, n, Q, ld, cb, mine_cols, lists[g], nodes, rb, g, l, red, [&](int ri) {
        const int row = rb * 32 + g * RPG + ri;
        if (row < n) tiled_max_store<OUT>(red[ri].s, red[ri].had, row, cb, N, qp, flip, out);
    });
}

// ---- the column view: out = max over A_tiled^T's rows -----------------------------------------------------------------------------------
// tiled_u8_col_walk with the extremum, per chunk of 4 LPR output columns. Between rounds the state of the 128 x 4 LPR outputs is ONE
// dword a lane and output row (128 LPR 4 bytes: 32 KiB at 64 lanes) and a flag word a row.
template <int LPR, int OUT>
__global__ __launch_bounds__(256) void k_tiled_max_u8_t(const int64_t *__restrict__ col_ptr, const int64_t *__restrict__ col_tile,
                                                        const int32_t *__restrict__ col_rb, const uint32_t *__restrict__ tiles,
                                                        uint64_t n_tiles, int n, const uint8_t *__restrict__ Q, size_t ld, int N,
                                                        const float4 *__restrict__ qp, uint32_t flip, TiledMaxOut out, TiledNodes nodes) {
    constexpr int G = 256 / LPR, TS = TILED_T_TS;
    __shared__ __attribute__((aligned(16))) uint32_t mk[128 * TS];   // [tile column][staged tile]
    __shared__ int srb[TS];
    __shared__ uint32_t acc[128 * LPR];                              // [output row][lane]: four columns' running maximum
    __shared__ int any[128];                                         // whether an output row had a term
    __shared__ int lists[G][TILED_U8_CAP];
    const int q = blockIdx.x, tid = threadIdx.x;
    const int g = LPR == 64 ? __builtin_amdgcn_readfirstlane(tid / LPR) : tid / LPR;
    const int l = tid % LPR, cb = blockIdx.y * (LPR * 4) + l * 4;
    const bool mine_cols = cb < N;
    tiled_u8_col_walk<LPR>(col_ptr, col_tile, col_rb, tiles, n_tiles, n, Q, ld, cb, mine_cols, nodes, q, g, l, mk, srb, lists[g], acc, any,
                           TiledU8Extremum{0u, flip, false});

    for (int j = g; j < 128; j += G) {
        const int row = q * 128 + j;
        if (row >= n) break;
        tiled_max_store<OUT>(acc[j * LPR + l], any[j] != 0, row, cb, N, qp, flip, out);
    }
}

// the family as tiled_u8_launch takes it: the same three width classes on both views; its tail is (const float4 *qp, uint32_t flip,
// TiledMaxOut out)
template <int OUT>
struct TiledU8MaxKernels {
    static constexpr int COL_WIDEST = 64;
    template <int LPR> static auto row() { return k_tiled_max_u8<LPR, OUT>; }
    template <int LPR> static auto col() { return k_tiled_max_u8_t<LPR, OUT>; }
};

// ---- the entries' bodies, either view: invalid, then misaligned, then short, then the launch -----------------------------------------
template <class Index>
int tiled_max_raw_entry(const Index &ix, const TiledU8In &a, int is_min, int empty_code, uint8_t *out, size_t ldo, size_t out_bytes,
                        void *stream) {
    if (tiled_u8_invalid(ix, a) || !out || empty_code < 0 || empty_code > 255) return QGTC_EINVAL;
    if (tiled_u8_misaligned(a) || codes_matrix_misaligned(out, ldo, a.N)) return QGTC_EALIGN;
    if (tiled_u8_short(a) || out_bytes < codes_matrix_bytes(a.n, a.N, ldo)) return QGTC_ESIZE;
    const TiledMaxOut dst{out, ldo, nullptr, 0.0f, static_cast<uint32_t>(empty_code) * 0x01010101u};
    return tiled_u8_launch<TiledU8MaxKernels<TILED_MAX_RAW>>(ix, a, stream, static_cast<const float4 *>(nullptr), is_min ? 0xffffffffu : 0u,
                                                             dst);
}

template <class Index>
int tiled_max_affine_entry(const Index &ix, const TiledU8In &a, const float *qparams, int is_min, const CodesDest &d, void *stream) {
    if (tiled_u8_invalid(ix, a) || codes_dest_invalid(d) || !qparams) return QGTC_EINVAL;
    if (tiled_u8_misaligned(a) || codes_dest_misaligned(d, a.N) || !aligned16(qparams)) return QGTC_EALIGN;
    if (tiled_u8_short(a) || codes_dest_short(d, a.n, a.N)) return QGTC_ESIZE;
    const float4 *qp = reinterpret_cast<const float4 *>(qparams);
    const uint32_t flip = is_min ? 0xffffffffu : 0u;
    if (d.out) return tiled_u8_launch<TiledU8MaxKernels<TILED_MAX_FLOAT>>(ix, a, stream, qp, flip, TiledMaxOut{d.out, 0, nullptr, 0.0f, 0u});
    return tiled_u8_launch<TiledU8MaxKernels<TILED_MAX_CODES>>(ix, a, stream, qp, flip, TiledMaxOut{d.outq, d.ldo, d.qp(), d.qmax(), 0u});
}

}  // namespace
