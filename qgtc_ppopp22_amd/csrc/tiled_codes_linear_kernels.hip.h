// tiled_codes_linear_kernels.hip.h — part of libqgtc_hip.so (included by qgtc_tiled_codes_linear.hip, after common.hip.h,
// affine_kernels.hip.h, affine_linear_kernels.hip.h, affine_chain_kernels.hip.h and tiled_codes_kernels.hip.h): the middle walk of the
// static affine chain fused with the product behind it (include/qgtc_fused.h). One launch computes
//   codes( linear( codes( A . T ) ) )   or   linear( codes( A . T ) )
// on the row view: the byte-code walk of k_tiled_mm_u8<LPR, TILED_U8_CODES> re-quantises the 32 rows of its block under the
// intermediate's fixed row, and instead of storing them the workgroup multiplies them by W's codes on v_mfma_i32_16x16x64_i8 and runs the
// epilogue of k_affine_linear_q8. Everything between the two stages is integer-exact or fixed operation by operation, so the result is
// the composed route's, bit for bit.
//
// How the work is split. 256 threads, one workgroup per 32-row block, grid.y == 1: the workgroup holds the whole hidden width K (the
// walk's N), so K <= 4 LPR and K <= 256.
//   walk      LPR lanes a row group, RPG = LPR / 8 rows a group, lane l on the hidden columns 4 l .. 4 l + 3: the gather, its LDS
//             queues, node masks and term counters exactly as in k_tiled_mm_u8.
//   hand-over a lane's dword of four codes goes, XORed to signed bytes, to s_h[row][4 l] in LDS. Slots at k >= K are written 0 up to
//             PAD64(K), so the product and its row sums see nothing past K and no fragment needs a mask. All 32 rows are written: a row
//             past n carries the code of float +0. One barrier publishes s_h and the chunk of W staged ahead of the walk.
//   product   wave wv takes row tile wv & 1 (16 rows) and the column tiles t with t % 2 == wv >> 1 of the pass: NT accumulators a wave,
//             2 NT column tiles a pass. The A fragment of k-step s is the 16 bytes at s_h[16 (wv & 1) + fr][64 s + 16 fg], the natural
//             slot order of k_affine_linear_q8, so W's codes are staged as they lie (alin_stage<false>). The row sums come from one more
//             MFMA against ones. Where W does not fit beside s_h the column tiles are taken in passes; s_h is read again, never rebuilt.
//   epilogue  alin_epilogue per accumulator (its columns are 32 apart, so it is called a tile at a time): float32 out, or codes through
//             the quad transposition with the pad bytes of the code-matrix rule.
// Dynamic LDS: [32][PAD64(K) + 16] of s_h, then [32 NT][PAD64(K) + 16] of W; at most 48 KiB. Static: the walk's queues, 4 KiB.
#pragma once

namespace {

constexpr int TCL_LDS_BUDGET = ALIN_LDS_BUDGET;   // dynamic LDS of a workgroup, s_h and W's pass together

__host__ __device__ constexpr int tcl_pad64(int K) { return (K + 63) & ~63; }
__host__ __device__ constexpr size_t tcl_lds(int K, int NT) { return static_cast<size_t>(32 + 32 * NT) * (tcl_pad64(K) + ALIN_PAD); }

// the walk's operand and its re-quantiser
struct TclWalk {
    const uint8_t *Q;     // code matrix [n, K], rows ld bytes apart, under the row qp
    size_t ld;
    const float4 *qp;
    const float *row_scale;
    const float4 *hq;     // the intermediate's fixed row
    float hmax;
};

template <int LPR, int NT, bool OUTQ>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(NT <= 2 ? 8 : 1))) void k_tiled_mm_u8_lin(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ kquad,
                                                         const uint32_t *__restrict__ tiles, uint64_t n_tiles, int n, int K, TclWalk h,
                                                         AlinRight w, AlinOut o, TiledNodes nodes) {
    constexpr int G = 256 / LPR, RPG = 32 / G;   // row groups per workgroup, rows per group
    extern __shared__ __attribute__((aligned(16))) uint8_t s_dyn[];   // s_h [32][stride], then s_w [32 NT][stride]
    __shared__ int lists[G][RPG][TILED_U8_CAP];
    const int rb = blockIdx.x, tid = threadIdx.x;
    const int stride = tcl_pad64(K) + ALIN_PAD;
    uint8_t *s_h = s_dyn, *s_w = s_dyn + 32 * stride;
    const int tiles_n = (w.N + 15) >> 4;
    const uint8_t *__restrict__ Q = h.Q;
    const size_t ld = h.ld;

    // W's first pass, ahead of the walk: nothing of the walk touches s_w, and the hand-over's barrier publishes it
    alin_stage<false>(s_w, stride, w.wt, w.ldk, w.N, 0, min(2 * NT, tiles_n), 0, stride - ALIN_PAD, tid);

    // ---- the walk of k_tiled_mm_u8<LPR, TILED_U8_CODES>, chunk 0, and the hand-over: the dword mode 2 would store, as signed bytes,
    // into s_h ---------------------------------------------------------------------------------------------------------------------------
    const int g = LPR == 64 ? __builtin_amdgcn_readfirstlane(tid / LPR) : tid / LPR;
    const int l = tid % LPR, cb = l * 4;
    const bool mine_cols = cb < K;
    TiledU8Sum red[RPG];
    tiled_u8_row_walk<LPR>(row_ptr, kquad, tiles, n_tiles, n, Q, ld, cb, mine_cols, lists[g], nodes, rb, g, l, red, [&](int ri) {
        const float4 gq = h.qp[0], og = h.hq[0];
        const long long z = static_cast<long long>(gq.y);
        const uint32_t zero = codes_quant(0.0f, og.z, og.y, h.hmax);   // a row past n: float +0
        const int r = g * RPG + ri, row = rb * 32 + r;
        const float rs = h.row_scale && row < n ? h.row_scale[row] : 1.0f;
        uint32_t word = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            uint32_t c = zero;
            if (row < n) c = codes_quant(tiled_u8_dequant(red[ri].s[k], red[ri].terms, z, gq.x, h.row_scale != nullptr, rs), og.z, og.y, h.hmax);
            word |= (cb + k < K ? c ^ 0x80u : 0u) << (8 * k);
        }
        if (cb < stride - ALIN_PAD) *reinterpret_cast<uint32_t *>(s_h + r * stride + cb) = word;
    });
    __syncthreads();

    // ---- the product and its epilogue, 2 NT column tiles a pass ----------------------------------------------------------------------
    const int lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, fg = lane >> 4;
    const int half = wv >> 1;   // which of a pass's column tiles: the odd or the even ones
    const int ksteps = (stride - ALIN_PAD) >> 6;
    const long long m0 = static_cast<long long>(rb) * 32 + 16 * (wv & 1);
    const uint8_t *al = s_h + (16 * (wv & 1) + fr) * stride + 16 * fg;
    const uint8_t *bl = s_w + (16 * half + fr) * stride + 16 * fg;
    const float4 qa = h.hq[0];
    for (int tb = 0; tb < tiles_n; tb += 2 * NT) {
        const int pt = min(2 * NT, tiles_n - tb);   // column tiles of this pass
        if (tb) {
            __syncthreads();   // every wave has read the pass before
            alin_stage<false>(s_w, stride, w.wt, w.ldk, w.N, 16 * tb, pt, 0, stride - ALIN_PAD, tid);
            __syncthreads();
        }
        const int nt = (pt - half + 1) >> 1;   // of them this wave's: tb + half, tb + half + 2, ..
        i32x4 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; t++) acc[t] = i32x4{0, 0, 0, 0};
        i32x4 rsum = i32x4{0, 0, 0, 0};
        for (int ks = 0; ks < ksteps; ks++)
            alin_step<NT>(acc, rsum, *reinterpret_cast<const i32x4 *>(al + 64 * ks), bl + 64 * ks, 2 * stride, nt);
#pragma unroll
        for (int t = 0; t < NT; t++) {
            if (t >= nt) continue;   // (uniform over the wave: every lane of it reaches the quad moves)
            const i32x4 one[1] = {acc[t]};
            alin_epilogue<1, OUTQ>(one, rsum, 1, m0, 16 * (tb + half + 2 * t), fr, fg, n, K, qa, w, o);
        }
    }
}

}  // namespace
