// qgtc_affine.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): uniform affine quantisation, the C entries
// of include/qgtc_affine.h over the kernels of affine_kernels.hip.h. Every entry checks, enqueues on the
// caller's stream and returns: no atomics, no host read, no allocation.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "qgtc_affine.h"

#include "common.hip.h"
#include "affine_kernels.hip.h"

namespace {

inline bool affine_bits_ok(int b) { return b >= 1 && b <= 8; }

// stage-1 workgroups of the per-tensor range: 4096 elements (four float4 a thread) each, 1024 at the most
inline unsigned tensor_parts(int H, int W) {
    const unsigned long long total = static_cast<unsigned long long>(H) * static_cast<unsigned long long>(W);
    const unsigned long long parts = (total + 4095u) / 4096u;
    return static_cast<unsigned>(parts < 1u ? 1u : (parts > 1024u ? 1024u : parts));
}
// row slices of the per-column range: 32 rows a workgroup and pass, 64 slices at the most
inline int column_slices(int H) {
    const int rb = (H + 31) / 32;
    return rb < 1 ? 1 : (rb > 64 ? 64 : rb);
}

inline unsigned blocks_for(unsigned long long units, unsigned per_block, unsigned cap) {
    const unsigned long long b = (units + per_block - 1u) / per_block;
    return static_cast<unsigned>(b < 1u ? 1u : (b > cap ? cap : b));
}

template <class... P>
int affine_launch(void (*kern)(P...), dim3 grid, hipStream_t st, P... p) {
    void *params[] = {const_cast<void *>(static_cast<const void *>(&p))...};
    const hipError_t e = hipLaunchKernel(reinterpret_cast<const void *>(kern), grid, dim3(256), params, 0, st);
    return e == hipSuccess ? QGTC_OK : hip_fail(e, "hipLaunchKernel (affine)");
}

// one launch of 256-thread workgroups on `st`; the arguments are converted to the kernel's parameter types, and the status is the
// launch call's own return value (its text is kept for qgtc_last_hip_error)
template <class... P, class... A>
int affine_go(void (*kern)(P...), dim3 grid, hipStream_t st, A... a) {
    return affine_launch(kern, grid, st, static_cast<P>(a)...);
}
#define AFFINE_LAUNCH(...)                        \
    do {                                          \
        const int rc_ = affine_go(__VA_ARGS__);   \
        if (rc_ != QGTC_OK) return rc_;           \
    } while (0)

template <bool PERCOL>
int launch_pack(const float *x, int H, int W, int nbits, int col_major, const float4 *qp, uint32_t *out, hipStream_t st) {
    const float qmax = static_cast<float>((1 << nbits) - 1);
    if (!col_major) {
        const int rows_pad = pad8(H), row_words = step128(W) * 4;
        const unsigned long long units = static_cast<unsigned long long>(rows_pad) * ((row_words + 7) / 8);
        if ((W & 3) == 0 && aligned16(x) && units < (1ull << 30)) {
            // (the grids of qgtc_val2bit: two units in flight a wave while that covers the matrix, four beyond)
            if (units <= 8192u * 8u) {
                const unsigned g = blocks_for((units + 1) / 2, 4, 8192);
                AFFINE_LAUNCH(k_val2bit_affine_rows_v4<2, PERCOL>, dim3(g), st, x, H, W, nbits, qmax, qp, out, rows_pad, row_words, static_cast<int>(4u * g));
            } else {
                const unsigned g = blocks_for((units + 3) / 4, 4, 8192);
                AFFINE_LAUNCH(k_val2bit_affine_rows_v4<4, PERCOL>, dim3(g), st, x, H, W, nbits, qmax, qp, out, rows_pad, row_words, static_cast<int>(4u * g));
            }
        } else {
            const unsigned g = blocks_for(units, 4, 1u << 20);
            AFFINE_LAUNCH(k_val2bit_affine_rows<PERCOL>, dim3(g), st, x, H, W, nbits, qmax, qp, out, rows_pad, row_words, static_cast<int>(4u * g));
        }
    } else {
        const int lines = pad128(W), line_words = step128(H) * 4;
        const unsigned long long units = static_cast<unsigned long long>((lines + 63) / 64) * line_words;
        const unsigned g = blocks_for(units, 4, 8192);
        const int nw = static_cast<int>(4u * g);
        if (nbits <= 1)
            AFFINE_LAUNCH(k_val2bit_affine_cols<1, PERCOL>, dim3(g), st, x, H, W, nbits, qmax, qp, out, lines, line_words, nw);
        else if (nbits <= 2)
            AFFINE_LAUNCH(k_val2bit_affine_cols<2, PERCOL>, dim3(g), st, x, H, W, nbits, qmax, qp, out, lines, line_words, nw);
        else if (nbits <= 4)
            AFFINE_LAUNCH(k_val2bit_affine_cols<4, PERCOL>, dim3(g), st, x, H, W, nbits, qmax, qp, out, lines, line_words, nw);
        else
            AFFINE_LAUNCH(k_val2bit_affine_cols<8, PERCOL>, dim3(g), st, x, H, W, nbits, qmax, qp, out, lines, line_words, nw);
    }
    return QGTC_OK;
}

}  // namespace

size_t qgtc_affine_work_words(int H, int W, int per_column) {
    if (H <= 0 || W <= 0) return 0;
    return per_column ? 2u * static_cast<size_t>(column_slices(H)) * static_cast<size_t>(W) : 2u * static_cast<size_t>(tensor_parts(H, W));
}

int qgtc_affine_qparams(const float *x, int H, int W, int nbits, int per_column, float *qparams, size_t qparams_elems, uint32_t *work,
                        size_t work_words, void *stream) {
    if (!x || !qparams || !work || H <= 0 || W <= 0 || !affine_bits_ok(nbits)) return QGTC_EINVAL;
    if (!aligned16(qparams)) return QGTC_EALIGN;
    const size_t groups = per_column ? static_cast<size_t>(W) : 1u;
    if (qparams_elems < 4u * groups || work_words < qgtc_affine_work_words(H, W, per_column)) return QGTC_ESIZE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const float qmax = static_cast<float>((1 << nbits) - 1);
    if (per_column) {
        const int RB = column_slices(H);
        AFFINE_LAUNCH(k_affine_range_cols, dim3((W + 63) / 64, RB), st, x, H, W, work, RB);
        AFFINE_LAUNCH(k_affine_finish_cols, dim3((W + 255) / 256), st, static_cast<const uint32_t *>(work), W, RB, qmax, qparams);
    } else {
        const unsigned parts = tensor_parts(H, W);
        const unsigned long long total = static_cast<unsigned long long>(H) * static_cast<unsigned long long>(W);
        AFFINE_LAUNCH(k_affine_range_tensor, dim3(parts), st, x, total, aligned16(x) ? 1 : 0, work, parts * 256u);
        AFFINE_LAUNCH(k_affine_finish_tensor, dim3(1), st, static_cast<const uint32_t *>(work), static_cast<int>(parts), qmax, qparams);
    }
    return QGTC_OK;
}

int qgtc_val2bit_affine(const float *x, int H, int W, int nbits, int col_major, const float *qparams, int groups, uint32_t *out,
                        size_t out_words, int32_t *sums, size_t sums_elems, void *stream) {
    if (!x || !qparams || !out || H <= 0 || W <= 0 || !affine_bits_ok(nbits) || (groups != 1 && groups != W)) return QGTC_EINVAL;
    if (!aligned16(qparams) || !aligned16(out)) return QGTC_EALIGN;
    if (out_words < (col_major ? qgtc_cols_words(H, W, nbits, 0) : qgtc_rows_words(H, W, nbits))) return QGTC_ESIZE;
    const int n_lines = col_major ? W : H;
    if (sums && sums_elems < static_cast<size_t>(n_lines)) return QGTC_ESIZE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const float4 *qp = reinterpret_cast<const float4 *>(qparams);
    const int rc = groups == 1 ? launch_pack<false>(x, H, W, nbits, col_major, qp, out, st)
                               : launch_pack<true>(x, H, W, nbits, col_major, qp, out, st);
    if (rc != QGTC_OK) return rc;
    if (sums) {
        const int line_words = (col_major ? step128(H) : step128(W)) * 4;
        const size_t plane = static_cast<size_t>(col_major ? pad128(W) : pad8(H)) * line_words;
        int G = 4;   // lanes a line: within one wave up to 64 words a line, a whole workgroup beyond
        while (G < line_words && G < 64) G <<= 1;
        if (line_words > 64) G = 256;
        const unsigned per_block = 256u / static_cast<unsigned>(G);
        AFFINE_LAUNCH(k_affine_code_sums, dim3((static_cast<unsigned>(n_lines) + per_block - 1u) / per_block), st,
                      static_cast<const uint32_t *>(out), n_lines, line_words, nbits, plane, G, sums);
    }
    return QGTC_OK;
}

int qgtc_affine_dequant(const float *acc, int M, int N, int K, const float *qa, const int32_t *row_sums, const float *qb, int groups_b,
                        const int32_t *col_sums, const float *row_scale, const float *bias, int relu, float *out, size_t out_elems,
                        void *stream) {
    if (!acc || !qa || !qb || !out || M <= 0 || N <= 0 || K <= 0 || (groups_b != 1 && groups_b != N)) return QGTC_EINVAL;
    if (!aligned16(qa) || !aligned16(qb)) return QGTC_EALIGN;
    const unsigned long long total = static_cast<unsigned long long>(M) * static_cast<unsigned long long>(N);
    if (out_elems < total) return QGTC_ESIZE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const unsigned g = blocks_for(total, 256, 8192);
    AFFINE_LAUNCH(k_affine_dequant, dim3(g), st, acc, M, N, static_cast<long long>(K), reinterpret_cast<const float4 *>(qa), row_sums,
                  reinterpret_cast<const float4 *>(qb), groups_b == N && N > 1 ? 1 : 0, col_sums, row_scale, bias, relu ? 1 : 0, out,
                  g * 256u);
    return QGTC_OK;
}
