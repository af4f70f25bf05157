// affine_kernels.hip.h — part of libqgtc_hip.so (included by qgtc_affine.hip): uniform affine quantisation (include/qgtc_affine.h; DESIGN.md
// section 6.15o). The range reduction and its finish, the fused quantise + pack in both layouts, the code sums from the packed planes and
// the dequantising epilogue. The packers follow pack_kernels.hip.h (a float4 per lane and the 8-lane DPP OR in the rows layout; lane =
// column and register-assembled words in the cols layout); what differs is the quantiser, that an element outside the matrix must be
// given the code 0 explicitly (0.0f quantises to the zero point, not to 0), and that the parameters are read from device memory.
// Every float operation that the definition rounds is an __f*_rn intrinsic: hipcc contracts a * b + c into an FMA otherwise.
#pragma once

namespace {

constexpr float AFFINE_TINY = 0x1p-100f;   // scales below are replaced (qgtc_affine.h)

// ------------------------------------------------------------------------------------------
// the quantiser: one multiply, one v_rndne, one add, a clamp (and the select that sends a NaN to the zero point)
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t aquant(float x, float inv, float zp, float qmax) {
    const float y = __fmul_rn(x, inv);
    const float c = fminf(fmaxf(__fadd_rn(rintf(y), zp), 0.0f), qmax);
    return static_cast<uint32_t>(y != y ? zp : c);
}

// (lo, hi) of the finite elements seen so far, both starting at +0
__device__ __forceinline__ void range_take(float v, float &lo, float &hi) {
    const bool fin = fabsf(v) < __builtin_inff();   // false for NaN and +-inf
    lo = fin && v < lo ? v : lo;
    hi = fin && v > hi ? v : hi;
}

__device__ __forceinline__ void range_wave(float &lo, float &hi) {
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o));
        hi = fmaxf(hi, __shfl_xor(hi, o));
    }
}

// the four floats of a group from its (lo, hi); lo <= 0 <= hi, both finite
__device__ __forceinline__ float4 qparams_of(float lo, float hi, float qmax) {
    float scale = __fdiv_rn(__fsub_rn(hi, lo), qmax);
    if (scale < AFFINE_TINY) scale = hi == lo ? 1.0f : AFFINE_TINY;
    const float inv = __fdiv_rn(1.0f, scale);
    const float raw = rintf(__fmul_rn(-lo, inv));
    const float zp = fminf(raw > 0.0f ? raw : 0.0f, qmax);    // (a -0 or anything unordered becomes +0)
    return make_float4(scale, zp, inv, 0.0f);
}

// ------------------------------------------------------------------------------------------
// range, per tensor. Stage 1: a grid-stride pass, float4 loads where the base is 16-byte aligned, one (lo, hi) per workgroup into
// work[2 b], work[2 b + 1]. Stage 2: one workgroup folds the `parts` pairs and writes the group's row.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_affine_range_tensor(const float *__restrict__ x, unsigned long long total, int vec,
                                                             uint32_t *__restrict__ work, unsigned nthreads) {
    __shared__ float s_lo[4], s_hi[4];
    const unsigned long long t = blockIdx.x * 256ull + threadIdx.x;
    float lo = 0.0f, hi = 0.0f;
    if (vec) {
        const unsigned long long quads = total >> 2;
        const float4 *x4 = reinterpret_cast<const float4 *>(x);
        for (unsigned long long i = t; i < quads; i += nthreads) {
            const float4 v = x4[i];
            range_take(v.x, lo, hi);
            range_take(v.y, lo, hi);
            range_take(v.z, lo, hi);
            range_take(v.w, lo, hi);
        }
        const unsigned long long tail = (quads << 2) + t;    // at most three elements
        if (tail < total) range_take(x[tail], lo, hi);
    } else {
        for (unsigned long long i = t; i < total; i += nthreads) range_take(x[i], lo, hi);
    }
    range_wave(lo, hi);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_lo[wave] = lo;
        s_hi[wave] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        lo = fminf(fminf(s_lo[0], s_lo[1]), fminf(s_lo[2], s_lo[3]));
        hi = fmaxf(fmaxf(s_hi[0], s_hi[1]), fmaxf(s_hi[2], s_hi[3]));
        work[2u * blockIdx.x] = __float_as_uint(lo);
        work[2u * blockIdx.x + 1u] = __float_as_uint(hi);
    }
}

__global__ __launch_bounds__(256) void k_affine_finish_tensor(const uint32_t *__restrict__ work, int parts, float qmax,
                                                              float *__restrict__ qparams) {
    __shared__ float s_lo[4], s_hi[4];
    float lo = 0.0f, hi = 0.0f;
    for (int p = threadIdx.x; p < parts; p += 256) {
        lo = fminf(lo, __uint_as_float(work[2 * p]));
        hi = fmaxf(hi, __uint_as_float(work[2 * p + 1]));
    }
    range_wave(lo, hi);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_lo[wave] = lo;
        s_hi[wave] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        lo = fminf(fminf(s_lo[0], s_lo[1]), fminf(s_lo[2], s_lo[3]));
        hi = fmaxf(fmaxf(s_hi[0], s_hi[1]), fmaxf(s_hi[2], s_hi[3]));
        *reinterpret_cast<float4 *>(qparams) = qparams_of(lo, hi, qmax);
    }
}

// ------------------------------------------------------------------------------------------
// range, per column. Stage 1: workgroup (cb, rb) owns columns 64 cb .. 64 cb + 63; lane = column, so a wave reads 256 contiguous bytes of
// one row; its four waves take rows 4 (rb + k RB) + wave. The four partials meet in LDS; work[(rb W + c) 2 ..] gets the pair.
// Stage 2: one thread per column folds its RB pairs (adjacent threads read adjacent pairs) and writes the column's row.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_affine_range_cols(const float *__restrict__ x, int H, int W, uint32_t *__restrict__ work, int RB) {
    __shared__ float s_lo[4][64], s_hi[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane, rb = blockIdx.y;
    float lo = 0.0f, hi = 0.0f;
    if (c < W)
        for (long r = 4l * rb + wave; r < H; r += 4l * RB) range_take(x[static_cast<size_t>(r) * W + c], lo, hi);
    s_lo[wave][lane] = lo;
    s_hi[wave][lane] = hi;
    __syncthreads();
    if (wave == 0 && c < W) {
        lo = fminf(fminf(s_lo[0][lane], s_lo[1][lane]), fminf(s_lo[2][lane], s_lo[3][lane]));
        hi = fmaxf(fmaxf(s_hi[0][lane], s_hi[1][lane]), fmaxf(s_hi[2][lane], s_hi[3][lane]));
        const size_t at = (static_cast<size_t>(rb) * W + c) * 2u;
        work[at] = __float_as_uint(lo);
        work[at + 1u] = __float_as_uint(hi);
    }
}

__global__ __launch_bounds__(256) void k_affine_finish_cols(const uint32_t *__restrict__ work, int W, int RB, float qmax,
                                                            float *__restrict__ qparams) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= W) return;
    float lo = 0.0f, hi = 0.0f;
    for (int rb = 0; rb < RB; rb++) {
        const size_t at = (static_cast<size_t>(rb) * W + c) * 2u;
        lo = fminf(lo, __uint_as_float(work[at]));
        hi = fmaxf(hi, __uint_as_float(work[at + 1u]));
    }
    reinterpret_cast<float4 *>(qparams)[c] = qparams_of(lo, hi, qmax);
}

// the (zero_point, inv_scale) of column c, or of the tensor
template <bool PERCOL>
__device__ __forceinline__ void group_of(const float4 *__restrict__ qp, int c, int W, float &zp, float &inv) {
    const float4 g = qp[PERCOL ? (c < W ? c : 0) : 0];   // (per tensor: one address for the launch, a scalar load)
    zp = g.y;
    inv = g.z;
}

// ------------------------------------------------------------------------------------------
// val2bit_affine, rows layout, fast path (W % 4 == 0, 16-byte aligned x): k_val2bit_rows_v4's structure. A wave packs 256 columns of one
// row per unit: a float4 per lane, the nibble of its four columns per plane, eight adjacent lanes OR theirs into one word with DPP.
// ------------------------------------------------------------------------------------------
template <int UNROLL, bool PERCOL>
__global__ __launch_bounds__(256) void k_val2bit_affine_rows_v4(const float *__restrict__ x, int H, int W, int nbits, float qmax,
                                                                const float4 *__restrict__ qp, uint32_t *__restrict__ out, int rows_pad,
                                                                int row_words, int nwaves_i) {
    const uint32_t wave = (blockIdx.x * 256u + threadIdx.x) >> 6, nwaves = static_cast<uint32_t>(nwaves_i);
    const int lane = threadIdx.x & 63;
    const int chunks = (row_words + 7) >> 3;
    const uint32_t units = static_cast<uint32_t>(rows_pad) * chunks;   // < 2^30 (host-checked)
    const size_t plane = static_cast<size_t>(rows_pad) * row_words;
    const uint32_t sh_n = 28 - 4 * (lane & 7);
    float zp0, inv0;
    group_of<false>(qp, 0, W, zp0, inv0);
    for (uint32_t u0 = wave * UNROLL; u0 < units; u0 += nwaves * UNROLL) {
        float4 v[UNROLL];
        bool in[UNROLL];
        int rk[UNROLL], chk[UNROLL];
        rk[0] = static_cast<int>(u0 / chunks);
        chk[0] = static_cast<int>(u0 - static_cast<uint32_t>(rk[0]) * chunks);
#pragma unroll
        for (int k = 1; k < UNROLL; k++) {
            const bool wrap = chk[k - 1] + 1 == chunks;
            chk[k] = wrap ? 0 : chk[k - 1] + 1;
            rk[k] = wrap ? rk[k - 1] + 1 : rk[k - 1];
        }
#pragma unroll
        for (int k = 0; k < UNROLL; k++) {
            const int r = rk[k], c = chk[k] * 256 + lane * 4;
            v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
            in[k] = u0 + k < units && r < H && c < W;   // W % 4 == 0: the quad is entirely inside or outside
            if (in[k]) v[k] = *reinterpret_cast<const float4 *>(x + static_cast<size_t>(r) * W + c);
        }
#pragma unroll
        for (int k = 0; k < UNROLL; k++) {
            if (u0 + k >= units) break;  // wave-uniform
            const int r = rk[k], ch = chk[k], c = ch * 256 + lane * 4;
            uint32_t q0, q1, q2, q3;
            if (PERCOL) {
                float z, i;
                group_of<true>(qp, c, W, z, i);
                q0 = aquant(v[k].x, i, z, qmax);
                group_of<true>(qp, c + 1, W, z, i);
                q1 = aquant(v[k].y, i, z, qmax);
                group_of<true>(qp, c + 2, W, z, i);
                q2 = aquant(v[k].z, i, z, qmax);
                group_of<true>(qp, c + 3, W, z, i);
                q3 = aquant(v[k].w, i, z, qmax);
            } else {
                q0 = aquant(v[k].x, inv0, zp0, qmax);
                q1 = aquant(v[k].y, inv0, zp0, qmax);
                q2 = aquant(v[k].z, inv0, zp0, qmax);
                q3 = aquant(v[k].w, inv0, zp0, qmax);
            }
            // the four codes as one word, a byte each: outside the matrix the code is 0
            const uint32_t q = in[k] ? (q0 << 24) | (q1 << 16) | (q2 << 8) | q3 : 0u;
            const int wi = ch * 8 + (lane >> 3);
            uint32_t *dst = out + static_cast<size_t>(r) * row_words + wi;
            for (int p = 0; p < nbits; p++, dst += plane) {
                const uint32_t b = (q >> p) & 0x01010101u;                             // bit p of the four codes at bits 24, 16, 8, 0
                const uint32_t nib = ((b >> 21) | (b >> 14) | (b >> 7) | b) & 0xFu;    // -> bits 3, 2, 1, 0
                const uint32_t word = or_reduce8(nib << sh_n);
                if ((lane & 7) == 0 && wi < row_words) *dst = word;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// val2bit_affine, rows layout, any W and any 4-byte aligned x: k_val2bit_rows's structure. One wave per (row, 256-column chunk): four
// coalesced loads per lane, one ballot per (plane, load), lanes 0 .. 7 store the chunk's eight words.
// ------------------------------------------------------------------------------------------
template <bool PERCOL>
__global__ __launch_bounds__(256) void k_val2bit_affine_rows(const float *__restrict__ x, int H, int W, int nbits, float qmax,
                                                             const float4 *__restrict__ qp, uint32_t *__restrict__ out, int rows_pad,
                                                             int row_words, int nwaves_i) {
    const long wave = (static_cast<long>(blockIdx.x) * 256 + threadIdx.x) >> 6, nwaves = nwaves_i;
    const int lane = threadIdx.x & 63;
    const int chunks = (row_words + 7) >> 3;
    const long units = static_cast<long>(rows_pad) * chunks;
    const size_t plane = static_cast<size_t>(rows_pad) * row_words;
    for (long u = wave; u < units; u += nwaves) {
        const int r = static_cast<int>(u / chunks);
        const int ch = static_cast<int>(u % chunks);
        uint32_t q[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int c = ch * 256 + i * 64 + lane;
            float zp, inv;
            group_of<PERCOL>(qp, c, W, zp, inv);
            q[i] = (r < H && c < W) ? aquant(x[static_cast<size_t>(r) * W + c], inv, zp, qmax) : 0u;
        }
        const int wi = ch * 8 + lane;  // word this lane stores (lanes 0..7)
        for (int p = 0; p < nbits; p++) {
            unsigned long long m[4];
#pragma unroll
            for (int i = 0; i < 4; i++) m[i] = __ballot((q[i] >> p) & 1u);
            const int sel = (lane >> 1) & 3;
            const unsigned long long mm = sel == 0 ? m[0] : sel == 1 ? m[1] : sel == 2 ? m[2] : m[3];
            const uint32_t half = (lane & 1) ? static_cast<uint32_t>(mm >> 32) : static_cast<uint32_t>(mm);
            if (lane < 8 && wi < row_words) out[p * plane + static_cast<size_t>(r) * row_words + wi] = __brev(half);
        }
    }
}

// ------------------------------------------------------------------------------------------
// val2bit_affine, cols layout: k_val2bit_cols's structure. One wave per (64-column chunk, 32-row group): lane = column, 32 coalesced row
// reads in flight, each lane assembles its column's word per plane in registers. NB = compile-time bound on nbits.
// ------------------------------------------------------------------------------------------
template <int NB, bool PERCOL>
__global__ __launch_bounds__(256) void k_val2bit_affine_cols(const float *__restrict__ x, int H, int W, int nbits, float qmax,
                                                             const float4 *__restrict__ qp, uint32_t *__restrict__ out, int lines,
                                                             int line_words, int nwaves_i) {
    const long wave = (static_cast<long>(blockIdx.x) * 256 + threadIdx.x) >> 6, nwaves = nwaves_i;
    const int lane = threadIdx.x & 63;
    const int cchunks = (lines + 63) >> 6;
    const long units = static_cast<long>(cchunks) * line_words;
    const size_t plane = static_cast<size_t>(lines) * line_words;
    const bool small = units < (1l << 31);
    for (long u = wave; u < units; u += nwaves) {
        int cg, rw;   // (a 64-bit division by a run-time value only when the count needs it: launch-uniform)
        if (small) {
            const uint32_t u32 = static_cast<uint32_t>(u), q = u32 / static_cast<uint32_t>(cchunks);
            rw = static_cast<int>(q);
            cg = static_cast<int>(u32 - q * static_cast<uint32_t>(cchunks));
        } else {
            rw = static_cast<int>(u / cchunks);
            cg = static_cast<int>(u % cchunks);
        }
        const int c = cg * 64 + lane;
        float zp, inv;
        group_of<PERCOL>(qp, c, W, zp, inv);
        uint32_t wd[NB];
#pragma unroll
        for (int p = 0; p < NB; p++) wd[p] = 0u;
        float v[32];
#pragma unroll
        for (int rr = 0; rr < 32; rr++) {
            const int r = rw * 32 + rr;
            v[rr] = (r < H && c < W) ? x[static_cast<size_t>(r) * W + c] : 0.0f;
        }
#pragma unroll
        for (int rr = 0; rr < 32; rr++) {
            const uint32_t q = (rw * 32 + rr < H && c < W) ? aquant(v[rr], inv, zp, qmax) : 0u;   // outside the matrix the code is 0
#pragma unroll
            for (int p = 0; p < NB; p++) wd[p] |= ((q >> p) & 1u) << (31 - rr);
        }
        if (c < lines) {
#pragma unroll
            for (int p = 0; p < NB; p++)
                if (p < nbits) out[p * plane + static_cast<size_t>(c) * line_words + rw] = wd[p];
        }
    }
}

// ------------------------------------------------------------------------------------------
// the code sums from the packed planes: sums[l] = sum_p 2^p popcount(line l of plane p), for the first n_lines lines (the rows of the rows
// layout, the columns of the cols layout). Pad bits are 0, so the count is the sum of the line's codes exactly, whatever the order.
// G lanes share a line - a power of two from 4 to 64 (inside one wave), or 256 (the workgroup); a workgroup holds 256 / G lines. Lane j takes words j, j + G, .. of every plane.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_affine_code_sums(const uint32_t *__restrict__ bits, int n_lines, int line_words, int nbits,
                                                          size_t plane, int G, int32_t *__restrict__ sums) {
    __shared__ int s_part[4];
    const int j = threadIdx.x & (G - 1);
    const long line = static_cast<long>(blockIdx.x) * (256 / G) + threadIdx.x / G;
    int acc = 0;
    if (line < n_lines) {
        const uint32_t *base = bits + static_cast<size_t>(line) * line_words;
        for (int p = 0; p < nbits; p++, base += plane)
            for (int w = j; w < line_words; w += G) acc += __popc(base[w]) << p;
    }
    const int within = G < 64 ? G : 64;
    for (int o = within >> 1; o; o >>= 1) acc += __shfl_xor(acc, o);
    if (G == 256) {   // (launch-uniform) one line per workgroup: the four waves meet in LDS
        if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = acc;
        __syncthreads();
        acc = s_part[0] + s_part[1] + s_part[2] + s_part[3];
    }
    if (j == 0 && line < n_lines) sums[line] = acc;
}

// ------------------------------------------------------------------------------------------
// the dequantising epilogue, one thread per element (qgtc_affine.h). acc and out may be the same buffer: an element is read by the thread
// that writes it, before it writes.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_affine_dequant(const float *acc, int M, int N, long long K, const float4 *__restrict__ qa,
                                                        const int32_t *__restrict__ row_sums, const float4 *__restrict__ qb, int percol,
                                                        const int32_t *__restrict__ col_sums, const float *__restrict__ row_scale,
                                                        const float *__restrict__ bias, int relu, float *out, unsigned nthreads) {
    const unsigned long long total = static_cast<unsigned long long>(M) * N;
    const float4 a = qa[0];
    const long long za = static_cast<long long>(a.y);
    const bool small = total < (1ull << 32);
    for (unsigned long long idx = blockIdx.x * 256ull + threadIdx.x; idx < total; idx += nthreads) {
        int m, n;
        if (small) {
            const uint32_t i32 = static_cast<uint32_t>(idx), q = i32 / static_cast<uint32_t>(N);
            m = static_cast<int>(q);
            n = static_cast<int>(i32 - q * static_cast<uint32_t>(N));
        } else {
            m = static_cast<int>(idx / N);
            n = static_cast<int>(idx % N);
        }
        const float4 b = qb[percol ? n : 0];
        const long long zb = static_cast<long long>(b.y);
        long long t = static_cast<long long>(acc[idx]) + K * za * zb;
        if (row_sums) t -= zb * row_sums[m];
        if (col_sums) t -= za * col_sums[n];
        float o = __fmul_rn(static_cast<float>(t), __fmul_rn(a.x, b.x));
        if (row_scale) o = __fmul_rn(o, row_scale[m]);
        if (bias) o = __fadd_rn(o, bias[n]);
        if (relu) o = o > 0.0f ? o : 0.0f;
        out[idx] = o;
    }
}

}  // namespace
