// tiled_fanout.hip.h — part of libqgtc_hip.so (included by the _fanout units BEFORE the kernel headers): the fixed-fanout sample as a mask
// of the tile walk (include/qgtc_fanout.h). It is the edge-dropout test H(i, j, seed) >= T of tiled_drop.hip.h
// with a threshold per node of the sampled axis, thr[u], instead of one for the graph. Two forms, by whose thresholds thr holds:
//   own: the output rows' (a sample taken on the view the kernel walks). An output row gets the existing TiledDropRow<TV> with
//        T = thr[self], so the decoders run the code they run under edge dropout.
//   nbr: the neighbours' (a sample taken on the other view: every backward). kept(v) loads thr[v]; the decoders call it after their
//        v < n guard. With 64 lanes a row the address is wave-uniform.
// Like every mask it is the LAST element of the kernels' trailing pack; the kernels' own code does not change.
#pragma once

#include "tiled_drop.hip.h"

namespace {

// the nbr form as one output row sees it: TiledDropRow with the neighbour's threshold
template <bool TVIEW>
struct TiledFanoutNbrRow {
    uint32_t K, key, own;   // as in TiledDropRow
    const uint32_t *thr;
    __device__ __forceinline__ bool kept(int v) const {
        const uint32_t h = tiled_drop_mix32(static_cast<uint32_t>(v) ^ key) + (TVIEW ? 0u : TILED_DROP_GOLDEN);
        return tiled_drop_mix32((own ^ h) + K) >= thr[v];
    }
};

// what the launchers pass: the seed's words (d.T is unused), the thresholds and their length, tagged with the view and the form
template <bool TVIEW, bool NBR>
struct TiledFanoutView {
    TiledDrop d;
    const uint32_t *thr;
    int n;
};

template <bool TV>
struct tiled_is_drop<TiledFanoutNbrRow<TV>> { static constexpr bool value = true; };
template <bool TV, bool NBR>
struct tiled_is_drop<TiledFanoutView<TV, NBR>> { static constexpr bool value = true; };

// own: an output row past n has no cells (the format keeps them zero) but is still asked for its mask, so its threshold is not loaded
template <bool TV>
__device__ __forceinline__ TiledDropRow<TV> tiled_drop_for(int self, const TiledFanoutView<TV, false> &p) {
    const uint32_t s = static_cast<uint32_t>(self);
    return TiledDropRow<TV>{self < p.n ? p.thr[self] : 0u, p.d.K, TV ? p.d.k0 : p.d.k1,
                            TV ? tiled_drop_col_half(p.d, s) : tiled_drop_row_half(p.d, s)};
}
template <bool TV>
__device__ __forceinline__ TiledFanoutNbrRow<TV> tiled_drop_for(int self, const TiledFanoutView<TV, true> &p) {
    const uint32_t s = static_cast<uint32_t>(self);
    return TiledFanoutNbrRow<TV>{p.d.K, TV ? p.d.k0 : p.d.k1, TV ? tiled_drop_col_half(p.d, s) : tiled_drop_row_half(p.d, s), p.thr};
}

// ---- the host side of the _fanout entries ----------------------------------------------------------------------------------------------
// `rc` is the _drop twin's verdict on the shared arguments; the two causes of QGTC_EINVAL added here are reported with it, before any
// alignment refusal, and thr's alignment before any size refusal.
inline int tiled_fanout_args_ok(int rc, const uint32_t *thr, int thr_of_nbr) {
    if (rc == QGTC_EINVAL || !thr || (thr_of_nbr != 0 && thr_of_nbr != 1)) return QGTC_EINVAL;
    if (rc == QGTC_EALIGN || (reinterpret_cast<uintptr_t>(thr) & 3u) != 0) return QGTC_EALIGN;
    return rc;
}

// run(mask) with the mask of the form asked for on view TV
template <bool TV, class F>
int tiled_fanout_run(const uint32_t *thr, int thr_of_nbr, uint64_t seed, int n, F &&run) {
    const TiledDrop d = tiled_drop_make(0u, seed);
    return thr_of_nbr ? run(TiledFanoutView<TV, true>{d, thr, n}) : run(TiledFanoutView<TV, false>{d, thr, n});
}

}  // namespace
