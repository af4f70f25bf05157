// tiled_float_t_kernels.hip.h — part of libqgtc_hip.so (included by qgtc_tiled_float_t.hip and qgtc_tiled_float_t_src.hip, after
// tiled_t_kernels.hip.h and tiled_float_kernels.hip.h): the transposed float product of the tile-compressed adjacency,
// out = A_tiled^T . X (include/qgtc.h, "Float tiled products"; DESIGN.md sections 6.14, 6.15).
//
// One workgroup (256 threads) per k-quad q (output rows 128 q .. 128 q + 127) and chunk of LPR * CPL output columns. The k-quad's column
// list is walked in ascending tile order - ascending row block, so ascending neighbour id - TS = 8 tiles a round:
//   transpose  as in k_tiled_mm_t: each half-wave takes one tile (its list entry was loaded two rounds, its words one round ahead,
//              so that a round does not wait for them) and runs the 32 x 32 bit transpose on its 4 words; the masks (tile
//              column j over the tile's 32 rows, row i at bit 31 - i) go to LDS as [tile column][staged tile], so an output row
//              reads the round's 8 masks as two 16-byte words;
//   add        a ROW GROUP of LPR = 16 lanes owns the output rows j = g, g + 16, ...; lane l owns the columns chunk + l + cc * LPR,
//              cc < CPL (a wave thereby keeps the loads of 4 rows in flight). A row with a mask in this round takes its running sums
//              from LDS, decodes the staged tiles in order, each MSB first (ascending source row), adds the addressed rows of X in
//              that order and puts the sums back. The sums of the 128 x LPR * CPL outputs live in LDS between rounds because a row
//              is touched in few rounds and the row index is a loop variable; each word is read and written by one lane only.
// The rows are stored once at the end; SCALED multiplies by row_scale[row] first (one IEEE single multiply). The trailing pack `Src...`
// is tiled_float_kernels.hip.h's: empty, the kernel that existed; with src_scale, the shared adder scales every term by its source row;
// ending in the edge-dropout mask of this view (TiledDropView<true>), a dropped source row is never queued.
// Ending in the node masks (tiled_nodes.hip.h): the four row-bitmap words of k-quad q decide, from blockIdx
// alone and before the first barrier, whether the workgroup walks its list at all (none set: an empty list, so it stores its +0 rows and
// is done); in a live workgroup both bitmaps are ANDed into a tile's words as the transposer role loads them, BEFORE the bit transpose:
// lane `lane` holds tile row 31 - lane, neighbour rb * 32 + 31 - lane, whose bit of word rb of the neighbour bitmap is bit `lane`, and
// its four words cover the k-quad's 128 output rows in the bitmap's own bit order. The staged masks then hold participating neighbours
// of computed rows only: a masked-out output row has no mask in any round and is skipped by the add loop's zero test, and the decode
// sees no other bit. One dword per tile and half-wave, loaded with the tile's words one round ahead; nothing per neighbour.
// Ending in the edge values (tiled_edge.hip.h): a column mask does not say what lies left of a cell in its tile
// row, so the transposer role also keeps the round's raw words in LDS (8 tiles x 512 bytes), with each tile's val_ptr and its 32 val_row
// entries, loaded with the words one round ahead; the decoder then finds the slot of (tile row b, this column) from them.
#pragma once

namespace {

template <int LPR, int CPL, bool SCALED, class... Src>
__global__ __launch_bounds__(256) void k_tiled_mm_f32_t(const int64_t *__restrict__ col_ptr, const int64_t *__restrict__ col_tile,
                                                        const int32_t *__restrict__ col_rb, const uint32_t *__restrict__ tiles,
                                                        uint64_t n_tiles, int n, const float *__restrict__ X, int N,
                                                        const float *__restrict__ row_scale, float *__restrict__ out, Src... src) {
    constexpr int G = 256 / LPR, TS = TILED_T_TS;
    static_assert(TS == 8, "an output row reads its 8 masks of a round as two uint4");
    __shared__ __attribute__((aligned(16))) uint32_t mk[128 * TS];   // [tile column][staged tile]
    __shared__ int srb[TS];
    constexpr int W = LPR * CPL;   // output columns per workgroup
    __shared__ float acc[128 * W];
    __shared__ int lists[G][TILED_F32_CAP];
    constexpr bool EDGE = tiled_has_edge<Src...>();
    // with edge values: the slots of this row group's queued neighbours [TILED_F32_CAP]; the round's words before the transpose and their
    // val_row, [staged tile][tile row]; the staged tiles' val_ptr
    [[maybe_unused]] int *slots = nullptr, *evr = nullptr, *evp = nullptr;
    [[maybe_unused]] uint32_t *raw = nullptr;
    if constexpr (EDGE) {
        __shared__ int edge_slots[G][TILED_F32_CAP], edge_vr[TS * 32], edge_vp[TS];
        __shared__ __attribute__((aligned(16))) uint32_t edge_raw[TS * 32 * 4];
        slots = edge_slots[threadIdx.x / LPR];
        evr = edge_vr;
        evp = edge_vp;
        raw = edge_raw;
    }
    [[maybe_unused]] const TiledEdge ed = tiled_edge_of(src...);
    const int q = blockIdx.x, tid = threadIdx.x;
    const int g = LPR == 64 ? __builtin_amdgcn_readfirstlane(tid / LPR) : tid / LPR;
    const int l = tid % LPR, c0 = blockIdx.y * W + l;
    const int nrb = (n + 31) / 32;
    int *list = lists[g];
    for (int j = g; j < 128; j += G)
#pragma unroll
        for (int cc = 0; cc < CPL; ++cc) acc[j * W + cc * LPR + l] = 0.0f;

    const int lane = tid & 31, s_own = tid >> 5;   // transposer role: half-wave s of the workgroup stages tile base + s
    uint64_t b0 = 0, t1 = 0;                       // an adjacency without tiles may come without col_ptr
    constexpr bool NODES = tiled_has_nodes<Src...>();
    [[maybe_unused]] const TiledNodes nodes = tiled_nodes_of(src...);
    [[maybe_unused]] uint4 rw = make_uint4(0, 0, 0, 0);   // the row bitmap's words of this k-quad
    bool walk = n_tiles != 0;
    if constexpr (NODES) {
        rw = tiled_nodes_quad(nodes.row, q);
        walk = walk && (rw.x | rw.y | rw.z | rw.w) != 0;
    }
    if (walk) {
        b0 = static_cast<uint64_t>(col_ptr[q]);
        t1 = static_cast<uint64_t>(col_ptr[q + 1]);
        t1 = t1 < n_tiles ? t1 : n_tiles;
    }
    uint4 w = make_uint4(0, 0, 0, 0);
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
            uint4 r = *reinterpret_cast<const uint4 *>(tiles + t * 128 + (31 - lane) * 4);
            if constexpr (NODES) {
                const uint32_t nb = nodes.nbr ? nodes.nbr[rb] : 0xffffffffu;   // rb < S32(n) <= S128(n) * 4
                const uint32_t on = (nb >> lane) & 1u ? 0xffffffffu : 0u;
                r = make_uint4(r.x & rw.x & on, r.y & rw.y & on, r.z & rw.z & on, r.w & rw.w & on);
            }
            return r;
        }
        rb = -1;
        return make_uint4(0, 0, 0, 0);
    };
    // with edge values: val_row of this lane's tile row and the tile's val_ptr, after words() has checked the entry (rb < 0: none)
    [[maybe_unused]] int vr = 0, vp = 0;
    [[maybe_unused]] auto evals = [&](uint64_t t, int rb) {
        vr = vp = 0;
        if (rb >= 0) {
            vr = ed.val_row[t * 32 + (31 - lane)];
            vp = static_cast<int>(ed.val_ptr[t]);
        }
    };
    uint64_t tn;
    int rb, rbn;
    {
        uint64_t tc;
        entry(b0 + s_own, tc, rb);
        entry(b0 + TS + s_own, tn, rbn);
        w = words(tc, rb);
        if constexpr (EDGE) evals(tc, rb);
    }
    for (uint64_t base = b0; base < t1; base += TS) {
        {
            uint32_t v[4] = {w.x, w.y, w.z, w.w};
            if constexpr (EDGE) {
                *reinterpret_cast<uint4 *>(raw + (s_own * 32 + 31 - lane) * 4) = w;
                evr[s_own * 32 + 31 - lane] = vr;
                if (lane == 0) evp[s_own] = vp;
            }
            tiled_t_transpose(v, lane);
#pragma unroll
            for (int k = 0; k < 4; ++k) mk[(k * 32 + 31 - lane) * TS + s_own] = v[k];
            if (lane == 0) srb[s_own] = rb;
            rb = rbn;
            w = words(tn, rb);
            if constexpr (EDGE) evals(tn, rb);
            entry(base + 2 * TS + s_own, tn, rbn);
        }
        __syncthreads();
        for (int j = g; j < 128; j += G) {
            if (q * 128 + j >= n) break;
            const uint4 ma = *reinterpret_cast<const uint4 *>(mk + j * TS), mb = *reinterpret_cast<const uint4 *>(mk + j * TS + 4);
            const uint32_t m[TS] = {ma.x, ma.y, ma.z, ma.w, mb.x, mb.y, mb.z, mb.w};
            if (!(ma.x | ma.y | ma.z | ma.w | mb.x | mb.y | mb.z | mb.w)) continue;
            float s[CPL];
#pragma unroll
            for (int cc = 0; cc < CPL; ++cc) s[cc] = acc[j * W + cc * LPR + l];
            int cnt = 0;
#pragma unroll
            for (int st = 0; st < TS; ++st)
                if (m[st]) {
                    if constexpr (EDGE)
                        tiled_f32_decode<LPR, CPL>(m[st], srb[st] * 32, n, s, list, cnt, X, N, c0,
                                                   tiled_edge_for(TiledEdgeAtCol{slots, raw + st * 128, evr + st * 32, evp[st], j}, src)...);
                    else tiled_f32_decode<LPR, CPL>(m[st], srb[st] * 32, n, s, list, cnt, X, N, c0, tiled_drop_for(q * 128 + j, src)...);
                }
            if constexpr (EDGE) tiled_f32_add_rows<LPR, CPL>(s, list, cnt, X, N, c0, tiled_edge_for(TiledEdgeAtFlush{slots}, src)...);
            else tiled_f32_add_rows<LPR, CPL>(s, list, cnt, X, N, c0, src...);
#pragma unroll
            for (int cc = 0; cc < CPL; ++cc) acc[j * W + cc * LPR + l] = s[cc];
        }
        __syncthreads();
    }

    for (int j = g; j < 128; j += G) {
        const int row = q * 128 + j;
        if (row >= n) break;
        float sc = 1.0f;
        if constexpr (SCALED) sc = row_scale[row];
#pragma unroll
        for (int cc = 0; cc < CPL; ++cc) {
            const int c = c0 + cc * LPR;
            const float s = acc[j * W + cc * LPR + l];
            if (c < N) out[static_cast<uint64_t>(row) * N + c] = SCALED ? s * sc : s;
        }
    }
}

// ---- the launcher of k_tiled_mm_f32_t: tiled_mm_f32_launch on the column view (tiled_float_kernels.hip.h has the row view's and the
// templates the entries of both views share) ----------------------------------------------------------------------------------------------
template <bool SCALED, class... Pack>
int tiled_mm_f32_launch(const TiledColIndex &ix, const uint32_t *tiles, int64_t n_tiles, int n, const float *X, int N,
                        const float *row_scale, float *out, hipStream_t st, Pack... pack) {
    tiled_col_width_switch(N, [&](auto cpl) {
        constexpr int CPL = decltype(cpl)::value;
        hipLaunchKernelGGL((k_tiled_mm_f32_t<16, CPL, SCALED, Pack...>), tiled_col_grid(n, N, 16 * CPL), dim3(256), 0, st, ix.col_ptr,
                           ix.col_tile, ix.col_rb, tiles, static_cast<uint64_t>(n_tiles), n, X, N, row_scale, out, pack...);
    });
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

}  // namespace
