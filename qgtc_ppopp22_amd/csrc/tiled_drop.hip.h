// tiled_drop.hip.h — part of libqgtc_hip.so (included by tiled_float_kernels.hip.h, so by every float, extremum and attention unit):
// edge dropout inside the tile walk (include/qgtc.h, "Edge dropout"). Whether cell (i, j) of A survives is a
// pure function of (i, j, seed), so nothing per edge is stored and both views rebuild the same mask: on the column view the cell is still
// A's (row = the neighbour, column = the output row). All arithmetic is uint32 and wraps:
//     mix32(x):  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16
//     k0 = seed & 0xffffffff,  k1 = seed >> 32,  K = mix32(k0) + k1
//     R(i) = mix32(i ^ k0),  C(j) = mix32(j ^ k1) + 0x9E3779B9,  H = mix32((R(i) ^ C(j)) + K),  kept <=> H >= threshold
// The output row's half (R on the row view, C on the column view) is computed once per output row (TiledDropRow); a set bit then costs
// one mix32 of the neighbour's id, an xor, an add and one more mix32. Every lane of a row group computes the same decision from the same
// words; with 64 lanes a row the words are wave-uniform and the hash stays on the scalar unit.
//
// The kernels take the mask as the LAST element of their trailing template pack: no such element, and they are the kernels that existed
// (the helpers below are then constants and the instructions the same). The functions are __host__ __device__: qgtc_edge_kept is the
// same code on the host.
#pragma once

#include <cstdint>

namespace {

constexpr uint32_t TILED_DROP_GOLDEN = 0x9E3779B9u;

__host__ __device__ __forceinline__ uint32_t tiled_drop_mix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// the kernel argument: the threshold and the three words of the seed
struct TiledDrop {
    uint32_t T, k0, k1, K;
};

__host__ __device__ __forceinline__ TiledDrop tiled_drop_make(uint32_t threshold, uint64_t seed) {
    const uint32_t k0 = static_cast<uint32_t>(seed), k1 = static_cast<uint32_t>(seed >> 32);
    return TiledDrop{threshold, k0, k1, tiled_drop_mix32(k0) + k1};
}

__host__ __device__ __forceinline__ uint32_t tiled_drop_row_half(const TiledDrop &d, uint32_t i) { return tiled_drop_mix32(i ^ d.k0); }
__host__ __device__ __forceinline__ uint32_t tiled_drop_col_half(const TiledDrop &d, uint32_t j) {
    return tiled_drop_mix32(j ^ d.k1) + TILED_DROP_GOLDEN;
}
__host__ __device__ __forceinline__ bool tiled_drop_test(const TiledDrop &d, uint32_t r_half, uint32_t c_half) {
    return tiled_drop_mix32((r_half ^ c_half) + d.K) >= d.T;
}

// the mask as one output row sees it. TVIEW false: the output row is A's row i, the neighbour A's column; true: the output row is A's
// column j, the neighbour A's row.
template <bool TVIEW>
struct TiledDropRow {
    uint32_t T, K, key, own;   // key: the seed word of the neighbour's half; own: the output row's half
    __device__ __forceinline__ bool kept(int v) const {
        const uint32_t h = tiled_drop_mix32(static_cast<uint32_t>(v) ^ key) + (TVIEW ? 0u : TILED_DROP_GOLDEN);
        return tiled_drop_mix32((own ^ h) + K) >= T;
    }
};

template <bool TVIEW>
struct TiledDropView {   // what the launchers pass: the key, tagged with the view
    TiledDrop d;
};

// ---- what the shared templates ask of their trailing pack ----------------------------------------------------------------------------------
template <class T>
struct tiled_is_drop { static constexpr bool value = false; };
template <bool TV>
struct tiled_is_drop<TiledDropRow<TV>> { static constexpr bool value = true; };
template <bool TV>
struct tiled_is_drop<TiledDropView<TV>> { static constexpr bool value = true; };

// the elements of a pack that are not the mask (the source scale of the float product)
template <class... P>
constexpr int tiled_pack_operands() { return (0 + ... + (tiled_is_drop<P>::value ? 0 : 1)); }

// kept(v, pack...): true without a mask, the last element's decision with one
__device__ __forceinline__ bool tiled_drop_kept(int) { return true; }
template <class P0, class... P>
__device__ __forceinline__ bool tiled_drop_kept(int v, const P0 &p0, const P &...p) {
    if constexpr (tiled_is_drop<P0>::value) return p0.kept(v);
    else return tiled_drop_kept(v, p...);
}

// a pack element as output row `self` passes it on to the decoders: the mask gets the row's half of the hash, anything else is itself
template <class P>
__device__ __forceinline__ const P &tiled_drop_for(int, const P &p) { return p; }
template <bool TV>
__device__ __forceinline__ TiledDropRow<TV> tiled_drop_for(int self, const TiledDropView<TV> &p) {
    const uint32_t s = static_cast<uint32_t>(self);
    return TiledDropRow<TV>{p.d.T, p.d.K, TV ? p.d.k0 : p.d.k1, TV ? tiled_drop_col_half(p.d, s) : tiled_drop_row_half(p.d, s)};
}

}  // namespace
