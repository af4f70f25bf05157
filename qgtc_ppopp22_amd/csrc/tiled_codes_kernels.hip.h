// tiled_codes_kernels.hip.h — part of libqgtc_hip.so (included by qgtc_tiled_codes.hip and qgtc_tiled_codes_t.hip, after common.hip.h and
// bitmm_popcount.hip.h): the byte-code route of affine quantisation (include/qgtc_codes.h) - the quantiser to
// one byte a code, and the neighbour sum of a uint8 code matrix on the tile-compressed adjacency, on both views, under node masks, with
// the dequantising epilogue of qgtc_affine_dequant in the same launch.
//
// The walks are those of k_tiled_mm_f32 (tiled_float_kernels.hip.h) and k_tiled_mm_f32_t (tiled_float_t_kernels.hip.h): a tile is a
// compressed neighbour list, its set bits are decoded MSB first into an LDS queue of TILED_U8_CAP ids, and the addressed rows of the
// operand are loaded TILED_U8_AHEAD at a time. What differs:
//   - a lane owns FOUR ADJACENT columns and loads one dword per neighbour row (hence ld % 4 == 0 in the contract); a lane whose columns
//     all lie past N loads nothing, a dword that straddles N is loaded and its surplus sums are not stored;
//   - the sums are int32, one register per column, and each byte is added to its own: the compiler selects the bytes in the add itself
//     (v_add_u32_sdwa with a BYTE_k source on gfx950; DESIGN.md section 6.15p has the ISA that was read), so a dword costs four VALU
//     instructions and nothing has to be widened at a flush;
//   - integer sums are exact in any order: there is no add-order contract and the adds of a column are not one dependent chain per
//     neighbour beyond the accumulator itself; only the loads need run ahead;
//   - the decoder counts the ids it queues per output row: cnt[o], the degree under the masks, which the affine epilogue needs.
// The node masks are always compiled in (either pointer may be null: all nodes), through TiledNodesWalk<true> / tiled_nodes_quad.
#pragma once

#include "tiled_args.hip.h"
#include "tiled_nodes.hip.h"
#include "tiled_t_kernels.hip.h"   // the in-register bit transpose of the column view

namespace {

constexpr int TILED_U8_CAP = 32;    // decoded neighbour ids a row group queues in LDS before it adds their rows
constexpr int TILED_U8_AHEAD = 4;   // rows of Q whose loads are in flight before the first of them is added

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

// ---- the adder and the decoder both views share ---------------------------------------------------------------------------------------
// s[k] += Q[list[j]][cb + k], k < 4, for j = 0 .. cnt - 1. The loads of TILED_U8_AHEAD neighbours are issued together (past the end of the
// list the last entry is loaded again and not added). `mine`: the lane's first column lies inside N, otherwise it loads nothing. `list`
// lives in LDS and every lane of the row group wrote every entry itself, so no lane reads a word another lane produced.
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

// the set bits of `m`, MSB first, as neighbour ids base + (leading zeros), queued in `list` and counted in `terms`; ids from n up are
// dropped (the format keeps such cells zero; a foreign tile must not make the kernel read past Q). A full queue is added at once.
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

template <bool AFFINE>
__device__ __forceinline__ void tiled_u8_store(const int (&s)[4], int terms, int row, int cb, int N, const float4 *__restrict__ qp,
                                               const float *__restrict__ row_scale, void *__restrict__ out) {
    if constexpr (AFFINE) {
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

template <int LPR>
__device__ __forceinline__ uint32_t tiled_u8_bcast(uint32_t v, int src) {
    if constexpr (LPR == 64) return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), src));
    else return static_cast<uint32_t>(__shfl(static_cast<int>(v), src, LPR));
}

// ---- the row view: out = A_tiled . Q --------------------------------------------------------------------------------------------------
// One workgroup (256 threads) per 32-row block and chunk of 4 LPR output columns. A ROW GROUP of LPR lanes (16, 32 or a whole wave) owns
// RPG = 32 / (256 / LPR) output rows of the block, lane l on the columns chunk + 4 l .. 4 l + 3. The group walks the block's tiles once:
// lanes 0 .. RPG - 1 load the 16-byte tile rows of the group's rows (the next tile's while this one is decoded), every row's four words
// are broadcast, ANDed with the neighbour bitmap's words of the tile's k-quad (loaded one tile ahead) and decoded into that row's own
// queue. A workgroup whose word of the row bitmap is zero takes an empty tile range without reading row_ptr; a masked-out row of a live
// block does not load its tile rows. Every row of the block is stored once, through the epilogue.
template <int LPR, bool AFFINE>
__global__ __launch_bounds__(256) void k_tiled_mm_u8(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ kquad,
                                                     const uint32_t *__restrict__ tiles, uint64_t n_tiles, int n,
                                                     const uint8_t *__restrict__ Q, size_t ld, int N, const float4 *__restrict__ qp,
                                                     const float *__restrict__ row_scale, void *__restrict__ out, TiledNodes nodes) {
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
// One workgroup (256 threads) per k-quad q (output rows 128 q .. 128 q + 127) and chunk of W = 4 LPR output columns. The k-quad's column
// list is walked TS = 8 tiles a round, as in k_tiled_mm_f32_t: each half-wave loads one tile (its list entry two rounds, its words one
// round ahead), ANDs both bitmaps into the words and runs the 32 x 32 bit transpose; the column masks go to LDS as [tile column][staged
// tile]. A row group of LPR lanes owns the output rows j = g, g + G, ..; a row with a mask in this round takes its four sums and its term
// counter from LDS, decodes the staged tiles, adds the addressed rows of Q and puts sums and counter back: the running sums of the
// 128 x W outputs (int32, one int4 a lane) and the 128 counters beside them live in LDS between rounds; each word is read and written
// by the lanes of one row group only, and every lane of the group writes the counter (the same value to the same address). A k-quad whose
// four row-bitmap words are zero walks nothing and stores its rows through the epilogue with acc = cnt = 0.
template <int LPR, bool AFFINE>
__global__ __launch_bounds__(256) void k_tiled_mm_u8_t(const int64_t *__restrict__ col_ptr, const int64_t *__restrict__ col_tile,
                                                       const int32_t *__restrict__ col_rb, const uint32_t *__restrict__ tiles,
                                                       uint64_t n_tiles, int n, const uint8_t *__restrict__ Q, size_t ld, int N,
                                                       const float4 *__restrict__ qp, const float *__restrict__ row_scale,
                                                       void *__restrict__ out, TiledNodes nodes) {
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

// ---- the host side: lanes per output row by N, on both views -------------------------------------------------------------------------
// N up to 64: 16 lanes; up to 128: 32 lanes; beyond: a whole wave and chunks of 256 columns (grid.y). The column view keeps 128 x 4 LPR
// int32 sums in LDS, 128 KiB at 64 lanes, which leaves one workgroup a CU: it stops at 32 lanes (64 KiB) and takes chunks of 128.
template <class F>
void tiled_u8_width_switch(int N, int widest, F &&launch) {
    const int lanes = N <= 64 ? 16 : (N <= 128 || widest == 32 ? 32 : 64);
    switch (lanes) {
        case 16: launch(tiled_int<16>{}); break;
        case 32: launch(tiled_int<32>{}); break;
        default: launch(tiled_int<64>{}); break;
    }
}

template <bool AFFINE>
int tiled_u8_launch(const TiledRowIndex &ix, const uint32_t *tiles, int64_t n_tiles, int n, const uint8_t *Q, size_t ld, int N,
                    const float *qparams, const float *row_scale, void *out, const TiledNodes &nodes, hipStream_t st) {
    tiled_u8_width_switch(N, 64, [&](auto lpr) {
        constexpr int LPR = decltype(lpr)::value;
        hipLaunchKernelGGL((k_tiled_mm_u8<LPR, AFFINE>), dim3((n + 31) / 32, (N + LPR * 4 - 1) / (LPR * 4)), dim3(256), 0, st, ix.row_ptr,
                           ix.kquad, tiles, static_cast<uint64_t>(n_tiles), n, Q, ld, N, reinterpret_cast<const float4 *>(qparams), row_scale,
                           out, nodes);
    });
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

template <bool AFFINE>
int tiled_u8_launch(const TiledColIndex &ix, const uint32_t *tiles, int64_t n_tiles, int n, const uint8_t *Q, size_t ld, int N,
                    const float *qparams, const float *row_scale, void *out, const TiledNodes &nodes, hipStream_t st) {
    tiled_u8_width_switch(N, 32, [&](auto lpr) {
        constexpr int LPR = decltype(lpr)::value;
        if constexpr (LPR <= 32)
            hipLaunchKernelGGL((k_tiled_mm_u8_t<LPR, AFFINE>), dim3(step128(n), (N + LPR * 4 - 1) / (LPR * 4)), dim3(256), 0, st, ix.col_ptr,
                               ix.col_tile, ix.col_rb, tiles, static_cast<uint64_t>(n_tiles), n, Q, ld, N,
                               reinterpret_cast<const float4 *>(qparams), row_scale, out, nodes);
    });
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

// ---- the argument checks, made before any device work: invalid, then misaligned, then short ------------------------------------------
inline bool codes_aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
inline size_t codes_pad4(int W) { return (static_cast<size_t>(W) + 3u) & ~static_cast<size_t>(3); }
// the three rules of a code matrix [H, W]
inline bool codes_matrix_misaligned(const void *p, size_t ld, int W) {
    return !codes_aligned4(p) || ld < static_cast<size_t>(W) || (ld & 3u) != 0;
}
inline size_t codes_matrix_bytes(int H, int W, size_t ld) { return static_cast<size_t>(H - 1) * ld + codes_pad4(W); }

// either view; AFFINE wants qparams (16-byte aligned) and takes an optional row_scale
template <bool AFFINE, class Index>
int tiled_u8_entry(const Index &ix, const uint32_t *tiles, int64_t n_tiles, int n, const uint8_t *Q, size_t ld, size_t q_bytes, int N,
                   const float *qparams, const float *row_scale, void *out, size_t out_elems, const uint32_t *row_mask,
                   const uint32_t *nbr_mask, size_t mask_words, void *stream) {
    if (!Q || !out || N < 1 || (AFFINE && !qparams) || tiled_adj_malformed(ix.ok(), tiles, n_tiles, n)) return QGTC_EINVAL;
    if (tiled_adj_misaligned(tiles) || codes_matrix_misaligned(Q, ld, N) || !codes_aligned4(out) || !aligned16(qparams) ||
        !codes_aligned4(row_scale) || !aligned16(row_mask) || !aligned16(nbr_mask))
        return QGTC_EALIGN;
    if (q_bytes < codes_matrix_bytes(n, N, ld) || out_elems < static_cast<size_t>(n) * static_cast<size_t>(N)) return QGTC_ESIZE;
    if ((row_mask || nbr_mask) && mask_words < static_cast<size_t>(step128(n)) * 4) return QGTC_ESIZE;
    return tiled_u8_launch<AFFINE>(ix, tiles, n_tiles, n, Q, ld, N, qparams, row_scale, out, TiledNodes{row_mask, nbr_mask},
                                   static_cast<hipStream_t>(stream));
}

}  // namespace
