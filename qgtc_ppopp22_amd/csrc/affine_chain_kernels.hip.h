// affine_chain_kernels.hip.h — part of libqgtc_hip.so (included by qgtc_affine_chain.hip, after common.hip.h, affine_kernels.hip.h and
// affine_linear_kernels.hip.h): the products of the static affine chain (include/qgtc_chain.h). Two kernels on
// the split of k_affine_linear_u8 (four waves, 64 rows a workgroup, NT <= 16 accumulators on v_mfma_i32_16x16x64_i8, W's codes through
// LDS once per workgroup, the row sums from one more MFMA against ones), and the epilogue both share:
//   k_affine_linear_q8   the left operand is a uint8 code matrix in memory: no quantiser, one 16-byte load a lane and k-step, the natural
//                        slot order; the result goes out as float32 or as codes
//   k_affine_linear_u8q  the left operand is float32, quantised in registers exactly as k_affine_linear_u8 does; the result goes out as
//                        codes (float in, float out is k_affine_linear_u8 itself)
//   alin_epilogue        the dequantising epilogue of k_affine_linear_u8 per element, then either its float store or the quantiser of
//                        affine_kernels.hip.h (aquant) under the caller's fixed output row and a store of whole dwords of codes
//
// The code store. In the accumulator layout register `reg` of lane l = (fr, fg) is row 4 fg + reg, column 16 t + fr, so the four lanes of
// a quad (fr & ~3 .. fr | 3) hold a 4 x 4 block: four adjacent columns of four rows. A lane packs its four codes (one column, four
// rows) into a dword, the quad transposes the 4 x 4 bytes with three quad_perm DPP moves (lane j takes the dword of lane j + d and
// keeps its byte j), and lane j then holds the four adjacent codes of row 4 fg + j: one aligned dword store. A column past N carries the
// code 0 into the transposition, so the pad bytes of a row's last dword are written 0 by that same store, and a dword wholly past N is
// not stored. No LDS and no barrier: the K loop's last chunk of W need not be released first.
#pragma once

namespace {

// lane j of every quad reads lane (j + d) & 3 of its quad; all 64 lanes must be active
template <int D>
__device__ __forceinline__ uint32_t alin_quad_rot(uint32_t v) {
    constexpr int ctrl = ((0 + D) & 3) | (((1 + D) & 3) << 2) | (((2 + D) & 3) << 4) | (((3 + D) & 3) << 6);   // quad_perm
    return static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), ctrl, 0xf, 0xf, false));
}

// W's codes of lines n0 .. n0 + 16 nt - 1, k0 .. k0 + kl - 1 into LDS, shifted to signed: 16 bytes of a line per thread and turn. PERMUTE:
// the slot order of k_affine_linear_u8 (dword 4 j + i of a 64-byte block goes to dword 4 i + j); otherwise as they lie in memory, the
// order of a code matrix's 16-byte loads. Past N or past ldk: zeros, read by no live slot.
template <bool PERMUTE>
__device__ __forceinline__ void alin_stage(uint8_t *s_w, int stride, const uint8_t *__restrict__ wt, size_t ldk, int N, int n0, int nt, int k0,
                                           int kl, int tid) {
    const int upl = kl >> 4, units = 16 * nt * upl;
    for (int u = tid; u < units; u += 64 * ALIN_WAVES) {
        const int r = u / upl, c = u - r * upl;
        const int n = n0 + r;
        const size_t kb = static_cast<size_t>(k0) + 16u * c;
        u32x4 q = u32x4{0u, 0u, 0u, 0u};
        if (n < N && kb < ldk) q = *reinterpret_cast<const u32x4 *>(wt + static_cast<size_t>(n) * ldk + kb);   // ldk % 16 == 0
        q ^= u32x4{ALIN_SHIFT, ALIN_SHIFT, ALIN_SHIFT, ALIN_SHIFT};
        if constexpr (PERMUTE) {
            uint32_t *dst = reinterpret_cast<uint32_t *>(s_w + r * stride + (c >> 2) * 64) + (c & 3);
            dst[0] = q.x, dst[4] = q.y, dst[8] = q.z, dst[12] = q.w;
        } else {
            *reinterpret_cast<u32x4 *>(s_w + r * stride + c * 16) = q;   // stride % 16 == 0
        }
    }
}

// the right-hand operand and the epilogue's vectors, as qgtc_linear.h defines them
struct AlinRight {
    const uint8_t *wt;
    size_t ldk;
    int N;
    const float4 *qb;
    int percol;
    const int32_t *col_sums;
    const float *row_scale, *bias;
    int relu;
};

// where the result goes: out float32 [M, N], or (OUTQ) the code matrix q under the row qp
struct AlinOut {
    float *out;
    uint8_t *q;
    size_t ldo;
    const float4 *qp;
    float qmax;
};

// one k-step of a wave: NT products and the row sums
template <int NT>
__device__ __forceinline__ void alin_step(i32x4 (&acc)[NT], i32x4 &rs, const i32x4 af, const uint8_t *bl, int stride, int nt) {
    const i32x4 ones = i32x4{0x01010101, 0x01010101, 0x01010101, 0x01010101};
#pragma unroll
    for (int t = 0; t < NT; t++)
        if (t < nt) {
            const i32x4 bf = *reinterpret_cast<const i32x4 *>(bl + t * 16 * stride);
            acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af, bf, acc[t], 0, 0, 0);
        }
    rs = __builtin_amdgcn_mfma_i32_16x16x64_i8(af, ones, rs, 0, 0, 0);
}

// the epilogue of qgtc_affine_dequant on the shifted identity (include/qgtc_linear.h), per element in registers, operation for operation
// that of k_affine_linear_u8; then the float store, or the code store of the header comment. Every lane of the wave arrives here.
template <int NT, bool OUTQ>
__device__ __forceinline__ void alin_epilogue(const i32x4 (&acc)[NT], const i32x4 rs, int nt, long long m0, int n0, int fr, int fg, int M, int K,
                                              const float4 a, const AlinRight &w, const AlinOut &o) {
    const int N = w.N;
    const long long za = static_cast<long long>(a.y) - 128;
    float oinv = 0.0f, ozp = 0.0f;
    if constexpr (OUTQ) {
        const float4 og = o.qp[0];
        oinv = og.z, ozp = og.y;
    }
#pragma unroll
    for (int t = 0; t < NT; t++) {
        if (t >= nt) continue;   // (uniform: nt is the workgroup's)
        const int n = n0 + 16 * t + fr;
        const int nc = n < N ? n : N - 1;   // a column past N computes on column N - 1 and stores nothing (codes: the byte 0)
        const float4 b = w.qb[w.percol ? nc : 0];
        const long long zb = static_cast<long long>(b.y) - 128;
        const long long fixed = static_cast<long long>(K) * za * zb - za * (static_cast<long long>(w.col_sums[nc]) - 128ll * K);
        const float scale = __fmul_rn(a.x, b.x);
        const float bv = w.bias ? w.bias[nc] : 0.0f;
        uint32_t pack = 0u;
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            const long long m = m0 + 4 * fg + reg;
            const long long mc = m < M ? m : M - 1;
            const long long tt = static_cast<long long>(acc[t][reg]) - zb * rs[reg] + fixed;
            float v = __fmul_rn(static_cast<float>(tt), scale);
            if (w.row_scale) v = __fmul_rn(v, w.row_scale[mc]);
            if (w.bias) v = __fadd_rn(v, bv);
            if (w.relu) v = v > 0.0f ? v : 0.0f;
            if constexpr (OUTQ) {
                pack |= (n < N ? aquant(v, oinv, ozp, o.qmax) : 0u) << (8 * reg);
            } else {
                if (m < M && n < N) o.out[static_cast<size_t>(m) * N + n] = v;
            }
        }
        if constexpr (OUTQ) {
            const int j = fr & 3, sh = 8 * j;
            uint32_t word = pack & (0xffu << sh);                                        // row j, column j of the block: byte j already
            word |= ((alin_quad_rot<1>(pack) >> sh) & 0xffu) << (8 * ((j + 1) & 3));     // row j of the lane that holds column j + 1
            word |= ((alin_quad_rot<2>(pack) >> sh) & 0xffu) << (8 * ((j + 2) & 3));
            word |= ((alin_quad_rot<3>(pack) >> sh) & 0xffu) << (8 * ((j + 3) & 3));
            const long long m = m0 + 4 * fg + j;
            const int c = n0 + 16 * t + (fr & ~3);
            if (m < M && c < N) *reinterpret_cast<uint32_t *>(o.q + static_cast<size_t>(m) * o.ldo + c) = word;   // ldo % 4 == 0
        }
    }
}

// ------------------------------------------------------------------------------------------
// the product on a code matrix. A k-step of a row is 64 bytes: lane (fr, fg) loads the 16 bytes at row * ldx + 64 s + 16 fg, the four lanes
// of a row one contiguous 64-byte run, and the load IS the fragment - slot 16 fg + i holds k = 64 s + 16 fg + i -, so W is staged as it
// lies. The fragment is shifted to signed and every slot at k >= K cleared after the shift: the product and the row sums see nothing of
// what bytes K .. ldx - 1 hold. Two k-steps (4 VGPRs each) are in flight ahead of the one multiplied.
// V16: ldx % 16 == 0 and a 16-byte aligned base, one 16-byte load; otherwise four dwords. Either way no byte at or past PAD4(K) of a row is
// touched - the last row of a code matrix owns no more -, so the lane whose 16 bytes straddle PAD4(K) loads its dwords singly.
// ------------------------------------------------------------------------------------------
template <int NT, bool V16, bool OUTQ>
__global__ __launch_bounds__(64 * ALIN_WAVES) void k_affine_linear_q8(const uint8_t *__restrict__ xq, size_t ldx, int M, int K,
                                                                      const float4 *__restrict__ qa, AlinRight w, AlinOut o, int kc) {
    extern __shared__ __attribute__((aligned(16))) uint8_t s_w[];   // [16 nt][kc + ALIN_PAD]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, fg = lane >> 4;
    const long long m0 = static_cast<long long>(blockIdx.x) * ALIN_ROWS + wv * 16;
    const int n0 = static_cast<int>(blockIdx.y) * 16 * NT;
    const int nt = min(NT, (w.N - n0 + 15) >> 4);
    const int stride = kc + ALIN_PAD;
    const int ksteps = (K + 63) >> 6, K4 = (K + 3) & ~3;
    // a row past M reads row M - 1 (valid memory) and is not stored
    const long long mr = m0 + fr < M ? m0 + fr : M - 1;
    const uint8_t *xr = xq + static_cast<size_t>(mr) * ldx + 16 * fg;

    auto load = [&](int s) {
        const int k = 64 * s + 16 * fg;
        u32x4 v = u32x4{0u, 0u, 0u, 0u};
        if (V16 && k + 16 <= K4) {
            v = *reinterpret_cast<const u32x4 *>(xr + 64 * s);
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++)
                if (k + 4 * i < K4) v[i] = *reinterpret_cast<const uint32_t *>(xr + 64 * s + 4 * i);
        }
        return v;
    };
    // the fragment of k-step s: signed bytes, 0 in every slot at k >= K
    auto fragment = [&](int s, const u32x4 v) {
        i32x4 af;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int left = K - (64 * s + 16 * fg + 4 * i);   // bytes of this dword inside K
            const uint32_t keep = left >= 4 ? 0xffffffffu : (left <= 0 ? 0u : (1u << (8 * left)) - 1u);
            af[i] = static_cast<int>((v[i] ^ ALIN_SHIFT) & keep);
        }
        return af;
    };

    i32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) acc[t] = i32x4{0, 0, 0, 0};
    i32x4 rs = i32x4{0, 0, 0, 0};
    u32x4 cur = load(0), nx1 = load(1);
    for (int k0 = 0; k0 < 64 * ksteps; k0 += kc) {
        const int kl = min(kc, 64 * ksteps - k0);
        __syncthreads();   // every wave has read the chunk before
        alin_stage<false>(s_w, stride, w.wt, w.ldk, w.N, n0, nt, k0, kl, tid);
        __syncthreads();
        for (int sl = 0; sl < (kl >> 6); sl++) {
            const int s = (k0 >> 6) + sl;
            const u32x4 nx2 = load(s + 2);   // (past the last k-step every dword is past PAD4(K): no load is issued)
            alin_step<NT>(acc, rs, fragment(s, cur), s_w + fr * stride + sl * 64 + fg * 16, stride, nt);
            cur = nx1;
            nx1 = nx2;
        }
    }
    alin_epilogue<NT, OUTQ>(acc, rs, nt, m0, n0, fr, fg, M, K, qa[0], w, o);
}

// ------------------------------------------------------------------------------------------
// float32 in, codes out: the load, the quantiser, the slot order (slot 16 fg + 4 j + i holds k = 64 s + 16 j + 4 fg + i) and the K loop of
// k_affine_linear_u8 (affine_linear_kernels.hip.h), so the accumulators are its accumulators, under the code-emitting epilogue.
// ------------------------------------------------------------------------------------------
template <int NT, bool VEC>
__global__ __launch_bounds__(64 * ALIN_WAVES) void k_affine_linear_u8q(const float *__restrict__ x, int M, int K, const float4 *__restrict__ qa,
                                                                       float qmax, AlinRight w, AlinOut o, int kc) {
    extern __shared__ __attribute__((aligned(16))) uint8_t s_w[];   // [16 nt][kc + ALIN_PAD]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, fg = lane >> 4;
    const long long m0 = static_cast<long long>(blockIdx.x) * ALIN_ROWS + wv * 16;
    const int n0 = static_cast<int>(blockIdx.y) * 16 * NT;
    const int nt = min(NT, (w.N - n0 + 15) >> 4);
    const int stride = kc + ALIN_PAD;
    const int ksteps = (K + 63) >> 6;
    const float4 a = qa[0];
    const float zp = a.y, inv = a.z;
    const long long mr = m0 + fr < M ? m0 + fr : M - 1;
    const float *xr = x + static_cast<size_t>(mr) * K + 4 * fg;

    auto load = [&](int s, float (&v)[16]) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int k = 64 * s + 16 * j + 4 * fg;
            if constexpr (VEC) {
                float4 f = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (k < K) f = *reinterpret_cast<const float4 *>(xr + 64 * s + 16 * j);   // K % 4 == 0: all four inside or none
                v[4 * j] = f.x, v[4 * j + 1] = f.y, v[4 * j + 2] = f.z, v[4 * j + 3] = f.w;
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++) v[4 * j + i] = k + i < K ? xr[64 * s + 16 * j + i] : 0.0f;
            }
        }
    };

    i32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) acc[t] = i32x4{0, 0, 0, 0};
    i32x4 rs = i32x4{0, 0, 0, 0};
    float cur[16], nxt[16];
    load(0, cur);
    for (int k0 = 0; k0 < 64 * ksteps; k0 += kc) {
        const int kl = min(kc, 64 * ksteps - k0);
        __syncthreads();
        alin_stage<true>(s_w, stride, w.wt, w.ldk, w.N, n0, nt, k0, kl, tid);
        __syncthreads();
        for (int sl = 0; sl < (kl >> 6); sl++) {
            const int s = (k0 >> 6) + sl;
            load(s + 1, nxt);
            i32x4 af;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int k = 64 * s + 16 * j + 4 * fg;
                uint32_t word = 0u;
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const uint32_t q = aquant(cur[4 * j + i], inv, zp, qmax) ^ 0x80u;
                    word |= ((VEC || k + i < K) ? q : 0u) << (8 * i);   // a k past K adds nothing to the product or to the row sum
                }
                af[j] = static_cast<int>((!VEC || k < K) ? word : 0u);
            }
            alin_step<NT>(acc, rs, af, s_w + fr * stride + sl * 64 + fg * 16, stride, nt);
#pragma unroll
            for (int e = 0; e < 16; e++) cur[e] = nxt[e];
        }
    }
    alin_epilogue<NT, true>(acc, rs, nt, m0, n0, fr, fg, M, K, a, w, o);
}

}  // namespace
