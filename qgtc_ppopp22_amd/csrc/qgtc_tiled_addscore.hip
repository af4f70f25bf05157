// qgtc_tiled_addscore.hip — translation unit of libqgtc_hip.so (compiled in parallel with the others): the additive edge score of GATv2,
// out[slot(i, j) * H + h] = ADDSCORE(A[i, head h], B[j, head h]; att[head h]) for every stored cell of the tile-compressed adjacency
// (include/qgtc_addscore.h). The kernel is k_tiled_sddmm_heads of qgtc_tiled_sddmm.hip with DOT's product
// replaced: the same walk, queues and slot arithmetic, the same lane mappings -
//   narrow, d <= 64   a head is an aligned group of P = next_pow2(d) lanes, 64 / P heads share register slot k; one term from +0 per
//                     lane, then the xor butterfly at distances P/2 .. 1;
//   wide, d > 64      a head takes the whole wave on CH = ceil(d / 64) slots of its own, lane l on the columns l + 64 cc of the head,
//                     added in that order, then the full butterfly -
// and the same register (NS > 0) and re-reading (NS = 0) paths. The lane's att columns are held beside its columns of A. A padding
// slot holds att = 0 and u = fl(0 + 0): its term is fl(0 * L(+0)) = +0, which changes no sum (a sum that starts at +0 is never -0). The
// narrow mapping with H = 1 is ADDSCORE itself - the butterfly's stages above P add +0 -, so one head needs no kernel of its own:
// every heads >= 1 takes the variant tests/tiled_heads_model.py sddmm_heads_variant names.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "qgtc_addscore.h"

#include "common.hip.h"
#include "tiled_float_kernels.hip.h"
#include "tiled_max_kernels.hip.h"   // tiled_static_for (templates only: nothing is instantiated here)
#include "tiled_attn_kernels.hip.h"  // the wave sum of DOT and the leaky relu (templates only)

namespace {

// how the heads lie on the wave: d columns a head, H heads, lg = log2(P) (narrow), CH slots a head (wide)
struct TiledAddShape {
    int d, H, lg, CH;
};

// the matrix column that lane l holds in slot k, or -1 where the slot is padding
template <bool WIDE>
__device__ __forceinline__ int tiled_add_col(const TiledAddShape &sh, int k, int l) {
    if constexpr (WIDE) {
        const int hd = k / sh.CH, c = l + 64 * (k - hd * sh.CH);
        return hd < sh.H && c < sh.d ? hd * sh.d + c : -1;
    } else {
        const int pc = l + 64 * k, hd = pc >> sh.lg, idx = pc & ((1 << sh.lg) - 1);
        return hd < sh.H && idx < sh.d ? hd * sh.d + idx : -1;
    }
}

// the xor butterfly within aligned groups of 1 << lg lanes, the largest distance first
__device__ __forceinline__ float tiled_add_group_sum(float t, int lg) {
    for (int h = (1 << lg) >> 1; h >= 1; h >>= 1) t += __shfl_xor(t, h, 64);
    return t;
}

// fl(t + fl(w * L(fl(x + y)))): four roundings, none fused
__device__ __forceinline__ float tiled_add_term(float t, float x, float y, float w, float slope) {
#pragma clang fp contract(off)
    const float u = x + y;
    return tiled_f32_mul_add(t, w, tiled_att_lrelu(u, slope));
}

// out[slots[j] * H + h] = ADDSCORE of head h of A[self] and B[list[j]] for the queue's entries; the loads of TILED_F32_AHEAD
// neighbours' rows are issued together. `col`: the lane's column of every slot; `w`: att at that column (+0 in padding); `head_end[k]`
// (wide): the head whose last slot is k, or -1.
template <int NS, bool WIDE>
__device__ __forceinline__ void tiled_addscore_rows(const float (&a)[NS ? NS : 1], const float (&w)[NS ? NS : 1], const int (&col)[NS ? NS : 1],
                                                    const int (&head_end)[NS ? NS : 1], const float *__restrict__ Arow,
                                                    const float *__restrict__ att, float slope, const int *list, const int *slots, int cnt,
                                                    const float *__restrict__ B, int N, const TiledAddShape &sh, int l,
                                                    float *__restrict__ out, int n_values) {
    constexpr int R = NS ? NS : 1;
    const int P = 1 << sh.lg;
    for (int j = 0; j < cnt; j += TILED_F32_AHEAD) {
        [[maybe_unused]] float b[TILED_F32_AHEAD][R];
        int v[TILED_F32_AHEAD], sl[TILED_F32_AHEAD];
        tiled_static_for<TILED_F32_AHEAD>([&](auto u) {
            const int i = j + u < cnt ? j + u : cnt - 1;
            v[u] = list[i];
            sl[u] = slots[i];
            if constexpr (NS != 0) {
                const float *__restrict__ row = B + static_cast<uint64_t>(v[u]) * N;
#pragma unroll
                for (int k = 0; k < R; ++k) b[u][k] = col[k] >= 0 ? row[col[k]] : 0.0f;
            }
        });
        tiled_static_for<TILED_F32_AHEAD>([&](auto u) {
            if (j + u < cnt) {
                const bool ok = static_cast<unsigned>(sl[u]) < static_cast<unsigned>(n_values);
                float *__restrict__ o = out + static_cast<uint64_t>(ok ? sl[u] : 0) * sh.H;
                const float *__restrict__ row = B + static_cast<uint64_t>(v[u]) * N;
                if constexpr (NS != 0 && WIDE) {
                    float t = 0.0f;
                    tiled_static_for<R>([&](auto k) {
                        t = tiled_add_term(t, a[k], b[u][k], w[k], slope);   // past d: + fl(0 * L(+0)), the same bits
                        if (head_end[k] >= 0) {   // wave-uniform
                            const float s = tiled_att_wave_sum(t);
                            if (l == 0 && ok) o[head_end[k]] = s;
                            t = 0.0f;
                        }
                    });
                } else if constexpr (NS != 0) {
                    tiled_static_for<R>([&](auto k) {
                        if (k * 64 < sh.H * P) {   // wave-uniform: a slot past the last head holds nothing
                            const float t = tiled_add_group_sum(tiled_add_term(0.0f, a[k], b[u][k], w[k], slope), sh.lg);
                            const int pc = l + 64 * k;
                            if ((pc & (P - 1)) == 0 && (pc >> sh.lg) < sh.H && ok) o[pc >> sh.lg] = t;
                        }
                    });
                } else if constexpr (WIDE) {
                    for (int hd = 0; hd < sh.H; ++hd) {
                        float t = 0.0f;
                        for (int c = l; c < sh.d; c += 64) t = tiled_add_term(t, Arow[hd * sh.d + c], row[hd * sh.d + c], att[hd * sh.d + c], slope);
                        t = tiled_att_wave_sum(t);
                        if (l == 0 && ok) o[hd] = t;
                    }
                } else {
                    for (int p0 = 0; p0 < sh.H * P; p0 += 64) {   // whole waves: every lane takes part in the exchange
                        const int pc = p0 + l, hd = pc >> sh.lg, idx = pc & (P - 1);
                        const bool in = hd < sh.H && idx < sh.d;
                        const int c = in ? hd * sh.d + idx : 0;
                        const float t = tiled_add_group_sum(
                            tiled_add_term(0.0f, in ? Arow[c] : 0.0f, in ? row[c] : 0.0f, in ? att[c] : 0.0f, slope), sh.lg);
                        if (idx == 0 && hd < sh.H && ok) o[hd] = t;
                    }
                }
            }
        });
    }
}

template <int NS, bool WIDE>
__global__ __launch_bounds__(256) void k_tiled_addscore(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ kquad,
                                                        const uint32_t *__restrict__ tiles, uint64_t n_tiles, int n,
                                                        const float *__restrict__ A, const float *__restrict__ B, int N,
                                                        const float *__restrict__ att, float slope, TiledAddShape sh,
                                                        const int64_t *__restrict__ val_ptr, const int16_t *__restrict__ val_row,
                                                        float *__restrict__ out, int n_values) {
    constexpr int RPG = 8, R = NS ? NS : 1;
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
    int col[R], head_end[R];
    float w[R];
#pragma unroll
    for (int k = 0; k < R; ++k) {
        col[k] = NS ? tiled_add_col<WIDE>(sh, k, l) : -1;
        head_end[k] = WIDE && (k + 1) % sh.CH == 0 && k / sh.CH < sh.H ? k / sh.CH : -1;
        w[k] = col[k] >= 0 ? att[col[k]] : 0.0f;
    }
    float own[RPG][R];
    int cnt[RPG];
    tiled_static_for<RPG>([&](auto ri) {
        cnt[ri] = 0;
        const int row = row0 + ri < n ? row0 + ri : n - 1;   // a row past n walks zero words (the format keeps them zero)
#pragma unroll
        for (int k = 0; k < R; ++k) own[ri][k] = col[k] >= 0 ? A[static_cast<uint64_t>(row) * N + col[k]] : 0.0f;
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
            const uint32_t wd[4] = {a.x, a.y, a.z, a.w};
            tiled_static_for<RPG>([&](auto ri) {
                const int row = row0 + ri < n ? row0 + ri : n - 1;
                const bool live = row0 + ri < n;
                int sb = vp + __builtin_amdgcn_readlane(vr, ri);
                tiled_static_for<4>([&](auto k) {
                    uint32_t m = live ? tiled_f32_bcast<64>(wd[k], ri) : 0u;
                    const int base = q * 128 + k * 32;
                    while (m) {
                        const int b = __builtin_clz(m);
                        m &= ~(0x80000000u >> b);
                        const int v = base + b;
                        if (v < n) {
                            lists[g][ri][cnt[ri]] = v;
                            slots[g][ri][cnt[ri]] = sb;
                            if (++cnt[ri] == TILED_F32_CAP) {
                                tiled_addscore_rows<NS, WIDE>(own[ri], w, col, head_end, A + static_cast<uint64_t>(row) * N, att, slope,
                                                              lists[g][ri], slots[g][ri], cnt[ri], B, N, sh, l, out, n_values);
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
        tiled_addscore_rows<NS, WIDE>(own[ri], w, col, head_end, A + static_cast<uint64_t>(row) * N, att, slope, lists[g][ri], slots[g][ri],
                                      cnt[ri], B, N, sh, l, out, n_values);
    });
}

}  // namespace

int qgtc_tiled_addscore_heads_f32(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n,
                                  const float *A, const float *B, size_t ab_elems, int N, const float *att, size_t att_elems,
                                  float negative_slope, const int64_t *val_ptr, const int16_t *val_row, float *out, size_t n_values,
                                  int heads, void *stream) {
    const TiledRowIndex ix{row_ptr, kquad};
    int rc = QGTC_OK;
    if (!A || !B || !att || (n_values && !out) || N < 1 || heads < 1 || N % heads != 0 || !(negative_slope >= 0.0f && negative_slope <= 1.0f) ||
        tiled_adj_malformed(ix.ok(), tiles, n_tiles, n))
        rc = QGTC_EINVAL;
    else if (tiled_adj_misaligned(tiles) || !aligned4(A) || !aligned4(B) || !aligned4(att) || !aligned4(out)) rc = QGTC_EALIGN;
    else if (ab_elems < static_cast<size_t>(n) * static_cast<size_t>(N) || att_elems < static_cast<size_t>(N)) rc = QGTC_ESIZE;
    rc = tiled_edge_rc(rc, tiled_edge_index_ok(val_ptr, val_row, n_tiles, n_values));
    if (rc != QGTC_OK) return rc;
    if (!n_tiles || !n_values) return QGTC_OK;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 block(256), grid((n + 31) / 32);
    const uint64_t nt = static_cast<uint64_t>(n_tiles);
    const int d = N / heads;
    int lg = 0;
    while ((1 << lg) < d && lg < 6) ++lg;
    const TiledAddShape sh{d, heads, lg, (d + 63) / 64};
    const bool wide = d > 64;
    // register slots: the padded width H * P in 64s (narrow), H * CH (wide, while H * d <= 256); 0: the re-reading path
    const int64_t need = wide ? (static_cast<int64_t>(N) <= 256 ? static_cast<int64_t>(heads) * sh.CH : 7)
                              : ((static_cast<int64_t>(heads) << lg) + 63) / 64;
    auto launch = [&](auto ns, auto w) {
        hipLaunchKernelGGL((k_tiled_addscore<decltype(ns)::value, decltype(w)::value>), grid, block, 0, st, ix.row_ptr, ix.kquad, tiles, nt, n,
                           A, B, N, att, negative_slope, sh, val_ptr, val_row, out, static_cast<int>(n_values));
    };
    using yes = std::true_type;
    using no = std::false_type;
    if (wide) {
        if (need <= 4) launch(tiled_int<4>{}, yes{});
        else if (need <= 6) launch(tiled_int<6>{}, yes{});
        else launch(tiled_int<0>{}, yes{});
    } else {
        if (need <= 1) launch(tiled_int<1>{}, no{});
        else if (need <= 2) launch(tiled_int<2>{}, no{});
        else if (need <= 4) launch(tiled_int<4>{}, no{});
        else launch(tiled_int<0>{}, no{});
    }
    HIP_TRY(hipGetLastError());
    return QGTC_OK;
}
