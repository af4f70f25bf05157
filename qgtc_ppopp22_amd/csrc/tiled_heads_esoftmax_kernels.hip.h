// tiled_heads_esoftmax_kernels.hip.h — part of libqgtc_hip.so (included by qgtc_tiled_esoftmax.hip and qgtc_tiled_esoftmax_t.hip,
// after tiled_esoftmax_kernels.hip.h, whose walks and float helpers it uses as they are): the edge softmax and its gradient for H
// heads in one launch (include/qgtc_heads.h), and the host side of the softmax for any number of heads -
// the argument checks and one entry body per operation, which sends one head to the single-head kernels. Logits, weights and
// gradients are float32 [n_values, H], head-minor; the statistics are [n, H].
//
// A lane owns one node AND HC heads h0 .. h0 + HC - 1 of it, h0 = blockIdx.y * HC: the walks of the single-head kernels visit the
// node's cells in the same order, and a pass reads the cell's HC adjacent values and keeps HC independent statistics, each folded by
// the single-head pass's own expression - so head h gets the bits of the single-head kernel on element [:, h]. HC is the largest of
// 4, 2, 1 that divides H: a walk decodes every tile once for HC heads, and a cell's values are one 4 HC-byte read. The column view
// keeps its batched slot loads (TILED_ESM_CAP slots a flush, HC values each).
#pragma once

namespace {

template <int HC>
struct TiledEsmVec {
    float x[HC];
};
template <int HC>
struct TiledEsmVec2 {
    float a[HC], g[HC];
};
// the HC values of slot s from head h0 on
template <int HC>
__device__ __forceinline__ TiledEsmVec<HC> tiled_esm_heads_load(const float *__restrict__ p, int s, int H, int h0) {
    const float *__restrict__ q = p + static_cast<uint64_t>(s) * H + h0;
    TiledEsmVec<HC> v;
#pragma unroll
    for (int k = 0; k < HC; ++k) v.x[k] = q[k];
    return v;
}

// TiledEsmFwd and its three passes, HC heads wide
template <int HC>
struct TiledEsmHeadsFwd {
    const float *__restrict__ logits;
    float *__restrict__ alpha;
    int H, h0;
    float m[HC], den[HC], inv[HC];
    bool first;
    __device__ __forceinline__ float weight(float l, int k) const { return tiled_att_exp(tiled_att_sub(l, m[k])); }
    __device__ __forceinline__ void finish() {
#pragma unroll
        for (int k = 0; k < HC; ++k) inv[k] = den[k] > 0.0f ? __fdiv_rn(1.0f, den[k]) : 0.0f;
    }
};
template <int HC>
struct TiledEsmHeadsMaxPass {
    TiledEsmHeadsFwd<HC> &st;
    using V = TiledEsmVec<HC>;
    __device__ __forceinline__ V load(int s) const { return tiled_esm_heads_load<HC>(st.logits, s, st.H, st.h0); }
    __device__ __forceinline__ void apply(int, V l) {
#pragma unroll
        for (int k = 0; k < HC; ++k) st.m[k] = st.first ? l.x[k] : (l.x[k] > st.m[k] ? l.x[k] : st.m[k]);   // the first of equal values wins
        st.first = false;
    }
};
template <int HC>
struct TiledEsmHeadsDenPass {
    TiledEsmHeadsFwd<HC> &st;
    using V = TiledEsmVec<HC>;
    __device__ __forceinline__ V load(int s) const { return tiled_esm_heads_load<HC>(st.logits, s, st.H, st.h0); }
    __device__ __forceinline__ void apply(int, V l) {
#pragma unroll
        for (int k = 0; k < HC; ++k) st.den[k] = tiled_esm_add(st.den[k], st.weight(l.x[k], k));
    }
};
template <int HC>
struct TiledEsmHeadsAlphaPass {
    TiledEsmHeadsFwd<HC> &st;
    using V = TiledEsmVec<HC>;
    __device__ __forceinline__ V load(int s) const { return tiled_esm_heads_load<HC>(st.logits, s, st.H, st.h0); }
    __device__ __forceinline__ void apply(int s, V l) {
        float *__restrict__ o = st.alpha + static_cast<uint64_t>(s) * st.H + st.h0;
#pragma unroll
        for (int k = 0; k < HC; ++k) o[k] = tiled_att_mul(st.weight(l.x[k], k), st.inv[k]);
    }
};
template <int HC>
__device__ __forceinline__ TiledEsmHeadsFwd<HC> tiled_esm_heads_fwd(const float *logits, float *alpha, int H) {
    TiledEsmHeadsFwd<HC> st{logits, alpha, H, static_cast<int>(blockIdx.y) * HC, {}, {}, {}, true};
#pragma unroll
    for (int k = 0; k < HC; ++k) st.m[k] = st.den[k] = st.inv[k] = 0.0f;
    return st;
}
template <int HC>
__device__ __forceinline__ void tiled_esm_heads_stats(const TiledEsmHeadsFwd<HC> &st, int node, float *__restrict__ m_out,
                                                      float *__restrict__ inv_out) {
    const uint64_t at = static_cast<uint64_t>(node) * st.H + st.h0;
#pragma unroll
    for (int k = 0; k < HC; ++k) {
        if (m_out) m_out[at + k] = st.m[k];
        if (inv_out) inv_out[at + k] = st.inv[k];
    }
}

// TiledEsmBwd and its two passes, HC heads wide
template <int HC>
struct TiledEsmHeadsBwd {
    const float *__restrict__ alpha;
    const float *__restrict__ g;
    float *__restrict__ out;
    int H, h0;
    float S[HC];
    __device__ __forceinline__ TiledEsmVec2<HC> load(int s) const {
        const TiledEsmVec<HC> a = tiled_esm_heads_load<HC>(alpha, s, H, h0), gg = tiled_esm_heads_load<HC>(g, s, H, h0);
        TiledEsmVec2<HC> v;
#pragma unroll
        for (int k = 0; k < HC; ++k) {
            v.a[k] = a.x[k];
            v.g[k] = gg.x[k];
        }
        return v;
    }
};
template <int HC>
struct TiledEsmHeadsSumPass {
    TiledEsmHeadsBwd<HC> &st;
    using V = TiledEsmVec2<HC>;
    __device__ __forceinline__ V load(int s) const { return st.load(s); }
    __device__ __forceinline__ void apply(int, V v) {
#pragma unroll
        for (int k = 0; k < HC; ++k) st.S[k] = tiled_esm_add(st.S[k], tiled_att_mul(v.a[k], v.g[k]));
    }
};
template <int HC>
struct TiledEsmHeadsOutPass {
    TiledEsmHeadsBwd<HC> &st;
    using V = TiledEsmVec2<HC>;
    __device__ __forceinline__ V load(int s) const { return st.load(s); }
    __device__ __forceinline__ void apply(int s, V v) {
        float *__restrict__ o = st.out + static_cast<uint64_t>(s) * st.H + st.h0;
#pragma unroll
        for (int k = 0; k < HC; ++k) o[k] = tiled_att_mul(v.a[k], tiled_att_sub(v.g[k], st.S[k]));
    }
};
template <int HC>
__device__ __forceinline__ TiledEsmHeadsBwd<HC> tiled_esm_heads_bwd(const float *alpha, const float *g, float *out, int H) {
    TiledEsmHeadsBwd<HC> st{alpha, g, out, H, static_cast<int>(blockIdx.y) * HC, {}};
#pragma unroll
    for (int k = 0; k < HC; ++k) st.S[k] = 0.0f;
    return st;
}

#ifndef QGTC_TILED_ESOFTMAX_T
template <int HC>
__global__ __launch_bounds__(256) void k_tiled_esoftmax_heads(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ kquad,
                                                              const uint32_t *__restrict__ tiles, uint64_t n_tiles, int n,
                                                              const int64_t *__restrict__ val_ptr, const int16_t *__restrict__ val_row,
                                                              const float *__restrict__ logits, float *__restrict__ alpha, int n_values,
                                                              float *__restrict__ m_out, float *__restrict__ inv_out, int H) {
    const TiledEsmRow w = tiled_esm_row_of(row_ptr, n_tiles, n);
    if (!w.live) return;
    TiledEsmHeadsFwd<HC> st = tiled_esm_heads_fwd<HC>(logits, alpha, H);
    tiled_esm_row_walk(kquad, tiles, val_ptr, val_row, w.t0, w.t1, w.r, n, n_values, TiledEsmHeadsMaxPass<HC>{st});
    tiled_esm_row_walk(kquad, tiles, val_ptr, val_row, w.t0, w.t1, w.r, n, n_values, TiledEsmHeadsDenPass<HC>{st});
    st.finish();
    tiled_esm_row_walk(kquad, tiles, val_ptr, val_row, w.t0, w.t1, w.r, n, n_values, TiledEsmHeadsAlphaPass<HC>{st});
    tiled_esm_heads_stats(st, w.row, m_out, inv_out);
}

template <int HC>
__global__ __launch_bounds__(256) void k_tiled_esoftmax_grad_heads(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ kquad,
                                                                   const uint32_t *__restrict__ tiles, uint64_t n_tiles, int n,
                                                                   const int64_t *__restrict__ val_ptr,
                                                                   const int16_t *__restrict__ val_row, const float *__restrict__ alpha,
                                                                   const float *__restrict__ g, float *__restrict__ out, int n_values,
                                                                   int H) {
    const TiledEsmRow w = tiled_esm_row_of(row_ptr, n_tiles, n);
    if (!w.live) return;
    TiledEsmHeadsBwd<HC> st = tiled_esm_heads_bwd<HC>(alpha, g, out, H);
    tiled_esm_row_walk(kquad, tiles, val_ptr, val_row, w.t0, w.t1, w.r, n, n_values, TiledEsmHeadsSumPass<HC>{st});
    tiled_esm_row_walk(kquad, tiles, val_ptr, val_row, w.t0, w.t1, w.r, n, n_values, TiledEsmHeadsOutPass<HC>{st});
}
#else
template <int HC>
__global__ __launch_bounds__(128) void k_tiled_esoftmax_heads_t(const int64_t *__restrict__ col_ptr, const int64_t *__restrict__ col_tile,
                                                                const int32_t *__restrict__ col_rb, const uint32_t *__restrict__ tiles,
                                                                uint64_t n_tiles, int n, const int64_t *__restrict__ val_ptr,
                                                                const int16_t *__restrict__ val_row, const float *__restrict__ logits,
                                                                float *__restrict__ alpha, int n_values, float *__restrict__ m_out,
                                                                float *__restrict__ inv_out, int H) {
    __shared__ TiledEsmStage lds;
    const TiledEsmCol w = tiled_esm_col_of(col_ptr, n_tiles, n);
    TiledEsmHeadsFwd<HC> st = tiled_esm_heads_fwd<HC>(logits, alpha, H);
    tiled_esm_col_walk(col_tile, col_rb, tiles, n_tiles, n, val_ptr, val_row, w.b0, w.t1, w.j, w.live, n_values, lds,
                       TiledEsmHeadsMaxPass<HC>{st});
    tiled_esm_col_walk(col_tile, col_rb, tiles, n_tiles, n, val_ptr, val_row, w.b0, w.t1, w.j, w.live, n_values, lds,
                       TiledEsmHeadsDenPass<HC>{st});
    st.finish();
    tiled_esm_col_walk(col_tile, col_rb, tiles, n_tiles, n, val_ptr, val_row, w.b0, w.t1, w.j, w.live, n_values, lds,
                       TiledEsmHeadsAlphaPass<HC>{st});
    if (w.live) tiled_esm_heads_stats(st, w.col, m_out, inv_out);
}

template <int HC>
__global__ __launch_bounds__(128) void k_tiled_esoftmax_grad_heads_t(const int64_t *__restrict__ col_ptr,
                                                                     const int64_t *__restrict__ col_tile,
                                                                     const int32_t *__restrict__ col_rb,
                                                                     const uint32_t *__restrict__ tiles, uint64_t n_tiles, int n,
                                                                     const int64_t *__restrict__ val_ptr,
                                                                     const int16_t *__restrict__ val_row, const float *__restrict__ alpha,
                                                                     const float *__restrict__ g, float *__restrict__ out, int n_values,
                                                                     int H) {
    __shared__ TiledEsmStage lds;
    const TiledEsmCol w = tiled_esm_col_of(col_ptr, n_tiles, n);
    TiledEsmHeadsBwd<HC> st = tiled_esm_heads_bwd<HC>(alpha, g, out, H);
    tiled_esm_col_walk(col_tile, col_rb, tiles, n_tiles, n, val_ptr, val_row, w.b0, w.t1, w.j, w.live, n_values, lds,
                       TiledEsmHeadsSumPass<HC>{st});
    tiled_esm_col_walk(col_tile, col_rb, tiles, n_tiles, n, val_ptr, val_row, w.b0, w.t1, w.j, w.live, n_values, lds,
                       TiledEsmHeadsOutPass<HC>{st});
}
#endif

// ---- the host side: one entry body per operation for both views and any number of heads -------------------------------------------------
constexpr int TILED_ESM_HEADS_MAX = 65535;   // the heads ride the grid's y dimension (H / HC rows of it)

// the argument checks, made before any device work: invalid before misaligned; `index_ok` as in tiled_adj_malformed. vec: the float
// arrays of n_values * heads elements (wanted when there are values); m / inv are optional. heads outside 1 .. TILED_ESM_HEADS_MAX is
// QGTC_EINVAL before every other refusal's kind is weighed
template <size_t K>
inline int tiled_esm_args_ok(bool index_ok, const uint32_t *tiles, int64_t n_tiles, int n, const int64_t *val_ptr, const int16_t *val_row,
                             size_t n_values, const float *const (&vec)[K], const float *m, const float *inv, int heads) {
    int rc = QGTC_OK;
    bool missing = false, off = false;
    for (const float *v : vec) {
        missing = missing || (n_values && !v);
        off = off || !aligned4(v);
    }
    if (missing || tiled_adj_malformed(index_ok, tiles, n_tiles, n)) rc = QGTC_EINVAL;
    else if (tiled_adj_misaligned(tiles) || off || !aligned4(m) || !aligned4(inv)) rc = QGTC_EALIGN;
    rc = tiled_edge_rc(rc, tiled_edge_index_ok(val_ptr, val_row, n_tiles, n_values));
    return heads < 1 || heads > TILED_ESM_HEADS_MAX ? QGTC_EINVAL : rc;
}

// m = +0 and inv = 0 for every (node, head): an adjacency without tiles (or values) has no owner with cells
inline int tiled_esm_no_cells(int n, int H, float *m, float *inv, hipStream_t st) {
    const size_t bytes = static_cast<size_t>(n) * static_cast<size_t>(H) * sizeof(float);
    if (m) HIP_TRY(hipMemsetAsync(m, 0, bytes, st));
    if (inv) HIP_TRY(hipMemsetAsync(inv, 0, bytes, st));
    return QGTC_OK;
}

// launch(HC as an integral constant, grid y): the largest of 4, 2, 1 heads a lane that divides H
template <class F>
void tiled_esm_heads_switch(int H, F &&launch) {
    if (H % 4 == 0) launch(tiled_int<4>{}, H / 4);
    else if (H % 2 == 0) launch(tiled_int<2>{}, H / 2);
    else launch(tiled_int<1>{}, H);
}

// the launches of this unit's view: one head is the single-head kernel, H heads the kernel of HC heads a lane over H / HC grid rows
#ifndef QGTC_TILED_ESOFTMAX_T
inline void tiled_esm_launch(const TiledRowIndex &ix, const uint32_t *tiles, uint64_t nt, int n, const int64_t *val_ptr, const int16_t *val_row,
                             const float *logits, float *alpha, int nv, float *m, float *inv, int H, hipStream_t st) {
    const dim3 grid((n + 255) / 256), block(256);
    if (H > 1) {
        tiled_esm_heads_switch(H, [&](auto hc, int gy) {
            hipLaunchKernelGGL((k_tiled_esoftmax_heads<decltype(hc)::value>), dim3(grid.x, gy), block, 0, st, ix.row_ptr, ix.kquad, tiles, nt, n,
                               val_ptr, val_row, logits, alpha, nv, m, inv, H);
        });
        return;
    }
    hipLaunchKernelGGL(k_tiled_esoftmax, grid, block, 0, st, ix.row_ptr, ix.kquad, tiles, nt, n, val_ptr, val_row, logits, alpha, nv, m, inv);
}
inline void tiled_esm_grad_launch(const TiledRowIndex &ix, const uint32_t *tiles, uint64_t nt, int n, const int64_t *val_ptr,
                                  const int16_t *val_row, const float *alpha, const float *g, float *out, int nv, int H, hipStream_t st) {
    const dim3 grid((n + 255) / 256), block(256);
    if (H > 1) {
        tiled_esm_heads_switch(H, [&](auto hc, int gy) {
            hipLaunchKernelGGL((k_tiled_esoftmax_grad_heads<decltype(hc)::value>), dim3(grid.x, gy), block, 0, st, ix.row_ptr, ix.kquad, tiles, nt,
                               n, val_ptr, val_row, alpha, g, out, nv, H);
        });
        return;
    }
    hipLaunchKernelGGL(k_tiled_esoftmax_grad, grid, block, 0, st, ix.row_ptr, ix.kquad, tiles, nt, n, val_ptr, val_row, alpha, g, out, nv);
}
#else
inline void tiled_esm_launch(const TiledColIndex &ix, const uint32_t *tiles, uint64_t nt, int n, const int64_t *val_ptr, const int16_t *val_row,
                             const float *logits, float *alpha, int nv, float *m, float *inv, int H, hipStream_t st) {
    const dim3 grid(step128(n)), block(128);
    if (H > 1) {
        tiled_esm_heads_switch(H, [&](auto hc, int gy) {
            hipLaunchKernelGGL((k_tiled_esoftmax_heads_t<decltype(hc)::value>), dim3(grid.x, gy), block, 0, st, ix.col_ptr, ix.col_tile, ix.col_rb,
                               tiles, nt, n, val_ptr, val_row, logits, alpha, nv, m, inv, H);
        });
        return;
    }
    hipLaunchKernelGGL(k_tiled_esoftmax_t, grid, block, 0, st, ix.col_ptr, ix.col_tile, ix.col_rb, tiles, nt, n, val_ptr, val_row, logits,
                       alpha, nv, m, inv);
}
inline void tiled_esm_grad_launch(const TiledColIndex &ix, const uint32_t *tiles, uint64_t nt, int n, const int64_t *val_ptr,
                                  const int16_t *val_row, const float *alpha, const float *g, float *out, int nv, int H, hipStream_t st) {
    const dim3 grid(step128(n)), block(128);
    if (H > 1) {
        tiled_esm_heads_switch(H, [&](auto hc, int gy) {
            hipLaunchKernelGGL((k_tiled_esoftmax_grad_heads_t<decltype(hc)::value>), dim3(grid.x, gy), block, 0, st, ix.col_ptr, ix.col_tile,
                               ix.col_rb, tiles, nt, n, val_ptr, val_row, alpha, g, out, nv, H);
        });
        return;
    }
    hipLaunchKernelGGL(k_tiled_esoftmax_grad_t, grid, block, 0, st, ix.col_ptr, ix.col_tile, ix.col_rb, tiles, nt, n, val_ptr, val_row,
                       alpha, g, out, nv);
}
#endif

// the forward's entry on either view: the refusals, the adjacency without cells, the launch
template <class Index>
int tiled_esm_entry(const Index &ix, const uint32_t *tiles, int64_t n_tiles, int n, const int64_t *val_ptr, const int16_t *val_row,
                    const float *logits, float *alpha, size_t n_values, float *m, float *inv, int heads, void *stream) {
    const float *const vec[] = {logits, alpha};
    const int rc = tiled_esm_args_ok(ix.ok(), tiles, n_tiles, n, val_ptr, val_row, n_values, vec, m, inv, heads);
    if (rc != QGTC_OK) return rc;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (!n_tiles || !n_values) return tiled_esm_no_cells(n, heads, m, inv, st);
    tiled_esm_launch(ix, tiles, static_cast<uint64_t>(n_tiles), n, val_ptr, val_row, logits, alpha, static_cast<int>(n_values), m, inv, heads, st);
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

// the gradient's
template <class Index>
int tiled_esm_grad_entry(const Index &ix, const uint32_t *tiles, int64_t n_tiles, int n, const int64_t *val_ptr, const int16_t *val_row,
                         const float *alpha, const float *g, float *out, size_t n_values, int heads, void *stream) {
    const float *const vec[] = {alpha, g, out};
    const int rc = tiled_esm_args_ok(ix.ok(), tiles, n_tiles, n, val_ptr, val_row, n_values, vec, nullptr, nullptr, heads);
    if (rc != QGTC_OK) return rc;
    if (!n_tiles || !n_values) return QGTC_OK;
    tiled_esm_grad_launch(ix, tiles, static_cast<uint64_t>(n_tiles), n, val_ptr, val_row, alpha, g, out, static_cast<int>(n_values), heads,
                          static_cast<hipStream_t>(stream));
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}

}  // namespace
