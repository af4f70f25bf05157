// affine_linear_kernels.hip.h — part of libqgtc_hip.so (included by qgtc_affine_linear.hip, after common.hip.h and affine_kernels.hip.h):
// the byte-code route of the affine linear layer (include/qgtc_linear.h). Two kernels: the weight preparation
// (range, qparams row, transposed byte codes, column sums of one output column per workgroup) and the fused product (float32 X read in
// the left-hand fragment shape, quantised in registers, v_mfma_i32_16x16x64_i8 against W's codes in LDS, dequantised in registers).
// The quantiser, the range fold and the qparams rule are the functions of affine_kernels.hip.h themselves (aquant, range_take,
// range_wave, qparams_of), so the codes and the rows cannot differ from those of the bit-plane route.
//
// The fragments (i8gemm_kernel.hip.h has the maps of the instruction): lane l = (fr, fg) = (l & 15, l >> 4) holds 16 bytes of A's row fr
// and of B's column fr, k-slots 16 fg .. 16 fg + 15; C/D register `reg` of lane l is row 4 fg + reg, column fr. The instruction sums over
// its 64 k-slots, so which k of the matrix sits in which slot is free as long as A and B agree. Here slot 16 fg + 4 j + i holds
//   k = 64 s + 16 j + 4 fg + i                 (s: the k-step, j < 4: the lane's j-th load, i < 4: the element of the load)
// - the j-th 16-byte load of the four lanes of a row covers 64 CONTIGUOUS bytes of that row, and the four loads a whole 256-byte k-step,
// instead of each lane reading 64 bytes of its own that a single load instruction touches 16 bytes at a time. W's codes are put into LDS
// in the same order while they are staged (a 4 x 4 transposition of the dwords of every 64-byte block), so the right-hand fragment stays
// one ds_read_b128.
#pragma once

namespace {

constexpr int ALIN_WAVES = 4;                   // waves of a workgroup; each owns 16 rows of X and of the output
constexpr int ALIN_ROWS = 16 * ALIN_WAVES;      // rows a workgroup owns
constexpr int ALIN_PAD = 16;                    // bytes between the lines of W in LDS beyond the chunk: the 16 lanes of a read hit 16 different 16-byte slots
constexpr int ALIN_LDS_BUDGET = 48 * 1024;      // bytes of LDS a workgroup may take: three workgroups a CU at the least
constexpr uint32_t ALIN_SHIFT = 0x80808080u;    // unsigned code -> signed byte, four at a time

// k of W a workgroup holds in LDS at a time for NT column sub-tiles (16 NT lines): a multiple of the k-step, 1024 at the most
__host__ __device__ constexpr int alin_chunk(int NT) {
    const int kc = (ALIN_LDS_BUDGET / (16 * NT) - ALIN_PAD) / 64 * 64;
    return kc > 1024 ? 1024 : kc;
}

// ------------------------------------------------------------------------------------------
// weight preparation: workgroup n owns output column n. Per tensor every workgroup folds the whole (small) matrix and workgroup 0
// writes the one row. The column's codes go out transposed, K contiguous, pad bytes 0; their sum meets in LDS.
// ------------------------------------------------------------------------------------------
template <bool PERCOL>
__global__ __launch_bounds__(256) void k_affine_pack_weight(const float *__restrict__ w, int K, int N, float qmax, float4 *__restrict__ qparams,
                                                            uint8_t *__restrict__ codes_t, size_t ldk, int32_t *__restrict__ col_sums) {
    __shared__ float s_lo[4], s_hi[4];
    __shared__ int s_sum[4];
    const int tid = threadIdx.x, wave = tid >> 6, n = blockIdx.x;
    float lo = 0.0f, hi = 0.0f;
    if (PERCOL) {
        for (int k = tid; k < K; k += 256) range_take(w[static_cast<size_t>(k) * N + n], lo, hi);
    } else {
        const size_t total = static_cast<size_t>(K) * N;
        for (size_t i = tid; i < total; i += 256) range_take(w[i], lo, hi);
    }
    range_wave(lo, hi);
    if ((tid & 63) == 0) {
        s_lo[wave] = lo;
        s_hi[wave] = hi;
    }
    __syncthreads();
    lo = fminf(fminf(s_lo[0], s_lo[1]), fminf(s_lo[2], s_lo[3]));
    hi = fmaxf(fmaxf(s_hi[0], s_hi[1]), fmaxf(s_hi[2], s_hi[3]));
    const float4 g = qparams_of(lo, hi, qmax);
    if (tid == 0 && (PERCOL || n == 0)) qparams[PERCOL ? n : 0] = g;
    int sum = 0;
    uint8_t *line = codes_t + static_cast<size_t>(n) * ldk;
    for (size_t k = tid; k < ldk; k += 256) {
        const uint32_t q = k < static_cast<size_t>(K) ? aquant(w[k * N + n], g.z, g.y, qmax) : 0u;
        line[k] = static_cast<uint8_t>(q);
        sum += static_cast<int>(q);
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) sum += __shfl_xor(sum, o);
    if ((tid & 63) == 0) s_sum[wave] = sum;
    __syncthreads();
    if (tid == 0) col_sums[n] = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
}

// ------------------------------------------------------------------------------------------
// the fused product. Workgroup (bx, by) owns rows 64 bx .. 64 bx + 63 and columns 256 by .. of the output - all of N up to 256 columns,
// in sub-tiles of 16; NT bounds the sub-tiles at compile time (the accumulators live in registers), nt <= NT is what this block has.
// W's codes pass through LDS once per workgroup, `kc` k at a time (all of K when it fits). A wave streams its 16 rows of X from global
// memory, one k-step (64 k) ahead of the one it multiplies. The row sums of X's shifted codes come from one more MFMA against a
// fragment of ones: its result is already in the accumulators' row layout, with no cross-lane move.
// VEC: K % 4 == 0 and a 16-byte aligned x, one float4 a load; otherwise four floats, each with its own bound.
// ------------------------------------------------------------------------------------------
template <int NT, bool VEC>
__global__ __launch_bounds__(64 * ALIN_WAVES) void k_affine_linear_u8(const float *__restrict__ x, int M, int K, const float4 *__restrict__ qa,
                                                                      float qmax, const uint8_t *__restrict__ wt, size_t ldk, int N,
                                                                      const float4 *__restrict__ qb, int percol,
                                                                      const int32_t *__restrict__ col_sums, const float *__restrict__ row_scale,
                                                                      const float *__restrict__ bias, int relu, float *__restrict__ out, int kc) {
    extern __shared__ __attribute__((aligned(16))) uint8_t s_w[];   // [16 nt][kc + ALIN_PAD]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, fg = lane >> 4;
    const long long m0 = static_cast<long long>(blockIdx.x) * ALIN_ROWS + wv * 16;
    const int n0 = static_cast<int>(blockIdx.y) * 16 * NT;
    const int nt = min(NT, (N - n0 + 15) >> 4);
    const int stride = kc + ALIN_PAD;
    const int ksteps = (K + 63) >> 6;
    const float4 a = qa[0];
    const float zp = a.y, inv = a.z;
    // a row past M reads row M - 1 (valid memory) and is not stored
    const long long mr = m0 + fr < M ? m0 + fr : M - 1;
    const float *xr = x + static_cast<size_t>(mr) * K + 4 * fg;

    // k-step s of this lane: v[4 j + i] = x[row][64 s + 16 j + 4 fg + i], 0 past K (such a slot's code is cleared below)
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
    const i32x4 ones = i32x4{0x01010101, 0x01010101, 0x01010101, 0x01010101};
    float cur[16], nxt[16];
    load(0, cur);
    for (int k0 = 0; k0 < 64 * ksteps; k0 += kc) {
        const int kl = min(kc, 64 * ksteps - k0);
        __syncthreads();   // every wave has read the chunk before
        // stage lines n0 .. n0 + 16 nt - 1, k0 .. k0 + kl - 1: 16 bytes of a line per thread and turn; dword d = 4 j + i of a 64-byte block
        // goes to dword 4 i + j (the slot order of the header comment), shifted to signed. Past N or past ldk: zeros, read by no live slot.
        const int upl = kl >> 4, units = 16 * nt * upl;
        for (int u = tid; u < units; u += 64 * ALIN_WAVES) {
            const int r = u / upl, c = u - r * upl;
            const int n = n0 + r;
            const size_t kb = static_cast<size_t>(k0) + 16u * c;
            u32x4 q = u32x4{0u, 0u, 0u, 0u};
            if (n < N && kb < ldk) q = *reinterpret_cast<const u32x4 *>(wt + static_cast<size_t>(n) * ldk + kb);   // ldk % 16 == 0
            uint32_t *dst = reinterpret_cast<uint32_t *>(s_w + r * stride + (c >> 2) * 64) + (c & 3);
            dst[0] = q.x ^ ALIN_SHIFT;
            dst[4] = q.y ^ ALIN_SHIFT;
            dst[8] = q.z ^ ALIN_SHIFT;
            dst[12] = q.w ^ ALIN_SHIFT;
        }
        __syncthreads();
        for (int sl = 0; sl < (kl >> 6); sl++) {
            const int s = (k0 >> 6) + sl;
            load(s + 1, nxt);   // (past the last k-step every slot is past K: no load is issued)
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
            const uint8_t *bl = s_w + fr * stride + sl * 64 + fg * 16;
#pragma unroll
            for (int t = 0; t < NT; t++)
                if (t < nt) {
                    const i32x4 bf = *reinterpret_cast<const i32x4 *>(bl + t * 16 * stride);
                    acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af, bf, acc[t], 0, 0, 0);
                }
            rs = __builtin_amdgcn_mfma_i32_16x16x64_i8(af, ones, rs, 0, 0, 0);
#pragma unroll
            for (int e = 0; e < 16; e++) cur[e] = nxt[e];
        }
    }

    // the epilogue of qgtc_affine_dequant on the shifted identity (include/qgtc_linear.h), per element in registers
    const long long za = static_cast<long long>(a.y) - 128;
#pragma unroll
    for (int t = 0; t < NT; t++) {
        const int n = n0 + 16 * t + fr;
        if (t < nt && n < N) {
            const float4 b = qb[percol ? n : 0];
            const long long zb = static_cast<long long>(b.y) - 128;
            const long long fixed = static_cast<long long>(K) * za * zb - za * (static_cast<long long>(col_sums[n]) - 128ll * K);
            const float scale = __fmul_rn(a.x, b.x);
            const float bv = bias ? bias[n] : 0.0f;
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const long long m = m0 + 4 * fg + reg;
                if (m < M) {
                    const long long tt = static_cast<long long>(acc[t][reg]) - zb * rs[reg] + fixed;
                    float o = __fmul_rn(static_cast<float>(tt), scale);
                    if (row_scale) o = __fmul_rn(o, row_scale[m]);
                    if (bias) o = __fadd_rn(o, bv);
                    if (relu) o = o > 0.0f ? o : 0.0f;
                    out[static_cast<size_t>(m) * N + n] = o;
                }
            }
        }
    }
}

}  // namespace
