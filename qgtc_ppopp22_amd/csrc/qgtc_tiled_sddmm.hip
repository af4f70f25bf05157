// qgtc_tiled_sddmm.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): one dot product per stored cell of
// the tile-compressed adjacency, out[slot(i, j)] = DOT(A[i], B[j]) (include/qgtc.h, "Edge values"). The walk
// and the dot are those of the attention's score gradient (tiled_attn_kernels.hip.h, k_tiled_att_grad): a wave owns 8 rows of a 32-row
// block and is whole on each of them, lane j on the columns j + 64 cc, the row of A in registers up to N = 256; a neighbour's dot is 64
// strided partial sums (one unfused multiply and add a column, in column order), then the xor butterfly. Here the dot is stored at the
// cell's slot instead of being folded: every slot is written exactly once, by lane 0 of the wave that owns its row - no atomics.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "qgtc.h"

#include "common.hip.h"
#include "tiled_float_kernels.hip.h"
#include "tiled_max_kernels.hip.h"   // tiled_static_for (templates only: nothing is instantiated here)
#include "tiled_attn_kernels.hip.h"  // the wave sum of DOT (templates only)

namespace {

// out[slots[j]] = DOT(A[self], B[list[j]]) for the queue's entries; the loads of TILED_F32_AHEAD neighbours' rows are issued together
template <bool REG>
__device__ __forceinline__ void tiled_sddmm_rows(const float (&a)[4], const float *__restrict__ Arow, const int *list, const int *slots,
                                                 int cnt, const float *__restrict__ B, int N, int l, float *__restrict__ out, int n_values) {
    for (int j = 0; j < cnt; j += TILED_F32_AHEAD) {
        [[maybe_unused]] float b[TILED_F32_AHEAD][4];
        int v[TILED_F32_AHEAD], sl[TILED_F32_AHEAD];
        tiled_static_for<TILED_F32_AHEAD>([&](auto u) {
            const int i = j + u < cnt ? j + u : cnt - 1;
            v[u] = list[i];
            sl[u] = slots[i];
            if constexpr (REG) {
                const float *__restrict__ row = B + static_cast<uint64_t>(v[u]) * N;
#pragma unroll
                for (int cc = 0; cc < 4; ++cc) b[u][cc] = l + cc * 64 < N ? row[l + cc * 64] : 0.0f;
            }
        });
        tiled_static_for<TILED_F32_AHEAD>([&](auto u) {
            if (j + u < cnt) {
                float t = 0.0f;
                if constexpr (REG) {
#pragma unroll
                    for (int cc = 0; cc < 4; ++cc) t = tiled_f32_mul_add(t, a[cc], b[u][cc]);   // past N: + fl(0 * 0), the same bits
                } else {
                    const float *__restrict__ row = B + static_cast<uint64_t>(v[u]) * N;
                    for (int c = l; c < N; c += 64) t = tiled_f32_mul_add(t, Arow[c], row[c]);
                }
                t = tiled_att_wave_sum(t);
                if (l == 0 && static_cast<unsigned>(sl[u]) < static_cast<unsigned>(n_values)) out[sl[u]] = t;
            }
        });
    }
}

template <bool REG>
__global__ __launch_bounds__(256) void k_tiled_sddmm(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ kquad,
                                                     const uint32_t *__restrict__ tiles, uint64_t n_tiles, int n,
                                                     const float *__restrict__ A, const float *__restrict__ B, int N,
                                                     const int64_t *__restrict__ val_ptr, const int16_t *__restrict__ val_row,
                                                     float *__restrict__ out, int n_values) {
    constexpr int RPG = 8;
    __shared__ int lists[4][RPG][TILED_F32_CAP];
    __shared__ int slots[4][RPG][TILED_F32_CAP];
    const int rb = blockIdx.x, tid = threadIdx.x;
    const int g = __builtin_amdgcn_readfirstlane(tid / 64), l = tid % 64;
    const int nq = step128(n);
    uint64_t t0 = 0, t1 = 0;
    if (n_tiles != 0) {
        t0 = static_cast<uint64_t>(row_ptr[rb]);
        t1 = static_cast<uint64_t>(row_ptr[rb + 1]);
        t1 = t1 < n_tiles ? t1 : n_tiles;
    }
    const int row0 = rb * 32 + g * RPG;
    float own[RPG][4];
    int cnt[RPG];
    tiled_static_for<RPG>([&](auto ri) {
        cnt[ri] = 0;
        const int row = row0 + ri < n ? row0 + ri : n - 1;   // a row past n walks zero words (the format keeps them zero)
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) own[ri][cc] = REG && l + cc * 64 < N ? A[static_cast<uint64_t>(row) * N + l + cc * 64] : 0.0f;
    });
    const int mine_row = g * RPG + (l < RPG ? l : 0);   // lane l < RPG: row g * RPG + l of every tile
    const uint32_t *mine = tiles + mine_row * 4;
    uint4 a = make_uint4(0, 0, 0, 0);
    int q = -1, vp = 0, vr = 0;
    if (t0 < t1) {
        q = kquad[t0];
        vp = static_cast<int>(val_ptr[t0]);
        if (l < RPG) {
            a = *reinterpret_cast<const uint4 *>(mine + t0 * 128);
            vr = val_row[t0 * 32 + mine_row];
        }
    }
    for (uint64_t t = t0; t < t1; ++t) {
        uint4 an = make_uint4(0, 0, 0, 0);
        int qn = -1, vpn = 0, vrn = 0;
        if (t + 1 < t1) {
            qn = kquad[t + 1];
            vpn = static_cast<int>(val_ptr[t + 1]);
            if (l < RPG) {
                an = *reinterpret_cast<const uint4 *>(mine + (t + 1) * 128);
                vrn = val_row[(t + 1) * 32 + mine_row];
            }
        }
        if (static_cast<unsigned>(q) < static_cast<unsigned>(nq)) {
            const uint32_t w[4] = {a.x, a.y, a.z, a.w};
            tiled_static_for<RPG>([&](auto ri) {
                const int row = row0 + ri < n ? row0 + ri : n - 1;
                const bool live = row0 + ri < n;
                int sb = vp + __builtin_amdgcn_readlane(vr, ri);
                tiled_static_for<4>([&](auto k) {
                    uint32_t m = live ? tiled_f32_bcast<64>(w[k], ri) : 0u;
                    const int base = q * 128 + k * 32;
                    while (m) {
                        const int b = __builtin_clz(m);
                        m &= ~(0x80000000u >> b);
                        const int v = base + b;
                        if (v < n) {
                            lists[g][ri][cnt[ri]] = v;
                            slots[g][ri][cnt[ri]] = sb;
                            if (++cnt[ri] == TILED_F32_CAP) {
                                tiled_sddmm_rows<REG>(own[ri], A + static_cast<uint64_t>(row) * N, lists[g][ri], slots[g][ri], cnt[ri], B, N, l,
                                                      out, n_values);
                                cnt[ri] = 0;
                            }
                        }
                        ++sb;
                    }
                });
            });
        }
        a = an;
        q = qn;
        vp = vpn;
        vr = vrn;
    }
    tiled_static_for<RPG>([&](auto ri) {
        const int row = row0 + ri < n ? row0 + ri : n - 1;
        tiled_sddmm_rows<REG>(own[ri], A + static_cast<uint64_t>(row) * N, lists[g][ri], slots[g][ri], cnt[ri], B, N, l, out, n_values);
    });
}

}  // namespace

int qgtc_tiled_sddmm_f32(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const float *A,
                         const float *B, size_t ab_elems, int N, const int64_t *val_ptr, const int16_t *val_row, float *out,
                         size_t n_values, void *stream) {
    const TiledRowIndex ix{row_ptr, kquad};
    int rc = QGTC_OK;
    if (!A || !B || (n_values && !out) || N < 1 || tiled_adj_malformed(ix.ok(), tiles, n_tiles, n)) rc = QGTC_EINVAL;
    else if (tiled_adj_misaligned(tiles) || !aligned4(A) || !aligned4(B) || !aligned4(out)) rc = QGTC_EALIGN;
    else if (ab_elems < static_cast<size_t>(n) * static_cast<size_t>(N)) rc = QGTC_ESIZE;
    rc = tiled_edge_rc(rc, tiled_edge_index_ok(val_ptr, val_row, n_tiles, n_values));
    if (rc != QGTC_OK) return rc;
    if (!n_tiles || !n_values) return QGTC_OK;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 block(256), grid((n + 31) / 32);
    const uint64_t nt = static_cast<uint64_t>(n_tiles);
    if (N <= 256)
        hipLaunchKernelGGL((k_tiled_sddmm<true>), grid, block, 0, st, row_ptr, kquad, tiles, nt, n, A, B, N, val_ptr, val_row, out,
                           static_cast<int>(n_values));
    else
        hipLaunchKernelGGL((k_tiled_sddmm<false>), grid, block, 0, st, row_ptr, kquad, tiles, nt, n, A, B, N, val_ptr, val_row, out,
                           static_cast<int>(n_values));
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}
