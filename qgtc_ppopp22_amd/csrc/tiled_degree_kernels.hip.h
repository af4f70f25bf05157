// tiled_degree_kernels.hip.h — part of libqgtc_hip.so (included by qgtc_tiled_scaled.hip): the degrees of a tile-compressed adjacency
// in both directions, their reciprocals and their inverse square roots (include/qgtc.h, "Scaled tiled products and degrees" and "Float
// tiled products"; DESIGN.md sections 6.13, 6.15). A degree is
// the number of set cells of a row (out) or a column (in) of the quantised adjacency: the number of terms of the product's sum.
#pragma once

namespace {

// out_deg[row]: one thread per row of a 32-row block sums the popcounts of its 4 words over the block's tiles (32 lanes read one
// 512-byte tile in one go). Every row below n is written with a plain store; the tiles the product skips are skipped here.
__global__ __launch_bounds__(256) void k_tiled_out_degree(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ kquad,
                                                          const uint32_t *__restrict__ tiles, uint64_t n_tiles, int n,
                                                          int32_t *__restrict__ out_deg) {
    const int nq = step128(n), nrb = (n + 31) / 32;
    for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < static_cast<int64_t>(nrb) * 32;
         i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        const int rb = static_cast<int>(i >> 5), r = static_cast<int>(i & 31);
        int deg = 0;
        if (n_tiles) {
            uint64_t t1 = static_cast<uint64_t>(row_ptr[rb + 1]);
            t1 = t1 < n_tiles ? t1 : n_tiles;
            for (uint64_t t = static_cast<uint64_t>(row_ptr[rb]); t < t1; ++t) {
                if (static_cast<unsigned>(kquad[t]) >= static_cast<unsigned>(nq)) continue;
                const uint4 a = *reinterpret_cast<const uint4 *>(tiles + t * 128 + r * 4);
                deg += __builtin_popcount(a.x) + __builtin_popcount(a.y) + __builtin_popcount(a.z) + __builtin_popcount(a.w);
            }
        }
        if (i < n) out_deg[i] = deg;
    }
}

// in_deg (cleared by the launcher): each half-wave takes one tile, lane l its row 31 - l, and runs the butterfly of k_tiled_mm_t on
// it; lane l then holds, for each word k, column 32 k + 31 - l as a mask over the tile's rows, whose popcount is that column's count
// in this tile. Non-zero counts are added with integer atomics: the result does not depend on the order in which they land.
__global__ __launch_bounds__(256) void k_tiled_in_degree(const int32_t *__restrict__ kquad, const uint32_t *__restrict__ tiles,
                                                         uint64_t n_tiles, int n, int32_t *__restrict__ in_deg) {
    const int nq = step128(n), lane = threadIdx.x & 31;
    const uint64_t per = blockDim.x >> 5, rounds = (n_tiles + per * gridDim.x - 1) / (per * gridDim.x);
    for (uint64_t k = 0; k < rounds; ++k) {   // the same trip count for every lane: the butterfly's shuffles need whole half-waves
        const uint64_t t = (k * gridDim.x + blockIdx.x) * per + (threadIdx.x >> 5);
        uint4 w = make_uint4(0, 0, 0, 0);
        int q = 0;
        if (t < n_tiles) {
            q = kquad[t];
            if (static_cast<unsigned>(q) < static_cast<unsigned>(nq)) w = *reinterpret_cast<const uint4 *>(tiles + t * 128 + (31 - lane) * 4);
        }
        uint32_t v[4] = {w.x, w.y, w.z, w.w};
        tiled_t_transpose(v, lane);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = q * 128 + j * 32 + 31 - lane, cnt = __builtin_popcount(v[j]);
            if (cnt && col < n) atomicAdd(in_deg + col, cnt);
        }
    }
}

// inv[i] = 1 / deg[i], correctly rounded; 0 where the degree is 0. Either pair may be absent.
__global__ void k_tiled_inv_degree(const int32_t *__restrict__ deg_a, float *__restrict__ inv_a, const int32_t *__restrict__ deg_b,
                                   float *__restrict__ inv_b, int n) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        if (inv_a) {
            const int d = deg_a[i];
            inv_a[i] = d ? __fdiv_rn(1.0f, static_cast<float>(d)) : 0.0f;
        }
        if (inv_b) {
            const int d = deg_b[i];
            inv_b[i] = d ? __fdiv_rn(1.0f, static_cast<float>(d)) : 0.0f;
        }
    }
}

// out[i] = fl32(1 / fl32(sqrt(fl32(deg[i])))): the conversion is exact (degrees are at most 2^23), the square root and the division are
// each correctly rounded (sqrtf and `/` are under hipcc's default; __fsqrt_rn is the approximate v_sqrt_f32 alone); 0 where the degree
// is 0. Plain stores.
__global__ void k_tiled_inv_sqrt_degree(const int32_t *__restrict__ deg, float *__restrict__ out, int n) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int d = deg[i];
        out[i] = d > 0 ? __fdiv_rn(1.0f, sqrtf(static_cast<float>(d))) : 0.0f;
    }
}

}  // namespace
