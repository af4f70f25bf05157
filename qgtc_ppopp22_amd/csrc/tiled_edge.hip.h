// tiled_edge.hip.h — part of libqgtc_hip.so (included by tiled_float_kernels.hip.h): a float32 value per stored cell of the tiled
// adjacency (include/qgtc.h, "Edge values"). The values lie in SLOT order - tile id, then tile row, then column
// ascending -, which depends on the tiles alone, so one array serves both views:
//     slot(t, r, c) = val_ptr[t] + val_row[t][r] + popcount(the bits of row r before column c)
// with val_ptr int64 [T + 1] the exclusive scan of the tiles' bit counts and val_row int16 [T, 32] the set bits of tile t above row r.
//
// The sum kernels take the values as the LAST element of their trailing template pack (TiledEdge): no such element, and every
// `if constexpr` below is discarded and the kernels are the ones that existed. A kernel turns the element into what ONE decode call
// needs (tiled_edge_for): on the row view the slot of the word's first bit, after which a set bit's slot is a running count
// (TiledEdgeRow); on the column view the staged tile's raw words, because a column mask does not say what lies left of the cell in its
// row (TiledEdgeCol). The decoder queues the slot beside the neighbour id and the adder loads values[slot] with the neighbour's row.
// Slots are kept as int: the entries that take n_values refuse one above 2^31 - 1.
#pragma once

#include <cstdint>
#include <initializer_list>
#include <type_traits>

namespace {

struct TiledEdge {   // the kernel argument
    const int64_t *val_ptr;
    const int16_t *val_row;
    const float *values;
    int n_values;
};

// the bits of word i (0 .. 3) of a tile row that lie before column c (0 .. 127): all of an earlier word, the top c & 31 bits of c's own
// word, none of a later one. A row's count is four ANDs and popcounts with these masks - no word is selected by a variable index:
// a conditional chain `k == 0 ? r.x : ... : r.w` on a uint4 read through a reference into LDS gave word 0 where word 3 was due when it
// was compiled into k_tiled_mm_f32_t for gfx950 (the same chain on registers, as in k_tiled_edge_slots' bit test, is fine).
__host__ __device__ __forceinline__ uint32_t tiled_edge_mask(int i, int c) {
    const int k = c >> 5;
    return i < k ? 0xffffffffu : i == k ? static_cast<uint32_t>(0xffffffff00000000ull >> (c & 31)) : 0u;
}
// the set bits of the tile row (x, y, z, w) before column c
__host__ __device__ __forceinline__ int tiled_edge_row_before(uint32_t x, uint32_t y, uint32_t z, uint32_t w, int c) {
    return __builtin_popcount(x & tiled_edge_mask(0, c)) + __builtin_popcount(y & tiled_edge_mask(1, c)) +
           __builtin_popcount(z & tiled_edge_mask(2, c)) + __builtin_popcount(w & tiled_edge_mask(3, c));
}

// what the shared adder needs of either view: the values and the queue of slots beside the queue of neighbours
struct TiledEdgeQueue {
    const float *values;
    int n_values;
    int *slots;
    __device__ __forceinline__ float value(int i) const {
        const int s = slots[i];
        return static_cast<unsigned>(s) < static_cast<unsigned>(n_values) ? values[s] : 0.0f;   // a foreign index reads nothing outside
    }
};
// row view: bit `b` of the decoded word is its k-th set bit, and `base` the slot of the first
struct TiledEdgeRow : TiledEdgeQueue {
    int base;
    __device__ __forceinline__ int slot(int, int k) const { return base + k; }
};
// column view: the decoded mask is column `col` of a staged tile over its 32 rows, bit b = tile row b; `raw` / `vrow` are the tile's
// words (four a row) and in-tile row prefix in LDS, `base` its val_ptr
struct TiledEdgeCol : TiledEdgeQueue {
    const uint32_t *raw;
    const int *vrow;
    int base, col;
    __device__ __forceinline__ int slot(int b, int) const {
        const uint32_t *r = raw + b * 4;
        return base + vrow[b] + tiled_edge_row_before(r[0], r[1], r[2], r[3], col);
    }
};

template <class T>
struct tiled_is_edge { static constexpr bool value = false; };
template <>
struct tiled_is_edge<TiledEdge> { static constexpr bool value = true; };
template <>
struct tiled_is_edge<TiledEdgeQueue> { static constexpr bool value = true; };
template <>
struct tiled_is_edge<TiledEdgeRow> { static constexpr bool value = true; };
template <>
struct tiled_is_edge<TiledEdgeCol> { static constexpr bool value = true; };

template <class... P>
constexpr bool tiled_has_edge() { return (false || ... || tiled_is_edge<P>::value); }

__device__ __forceinline__ TiledEdge tiled_edge_of() { return TiledEdge{nullptr, nullptr, nullptr, 0}; }
template <class P0, class... P>
__device__ __forceinline__ TiledEdge tiled_edge_of(const P0 &p0, const P &...p) {
    if constexpr (std::is_same<P0, TiledEdge>::value) return p0;
    else return tiled_edge_of(p...);
}

// where a decode call stands: the kernels build one of these per call, and a pack element that is not the values passes through
struct TiledEdgeAtRow {
    int *slots;
    int base;
};
struct TiledEdgeAtCol {
    int *slots;
    const uint32_t *raw;
    const int *vrow;
    int base, col;
};
struct TiledEdgeAtFlush {
    int *slots;
};
template <class At, class P>
__device__ __forceinline__ const P &tiled_edge_for(const At &, const P &p) { return p; }
__device__ __forceinline__ TiledEdgeRow tiled_edge_for(const TiledEdgeAtRow &at, const TiledEdge &e) {
    return TiledEdgeRow{{e.values, e.n_values, at.slots}, at.base};
}
__device__ __forceinline__ TiledEdgeCol tiled_edge_for(const TiledEdgeAtCol &at, const TiledEdge &e) {
    return TiledEdgeCol{{e.values, e.n_values, at.slots}, at.raw, at.vrow, at.base, at.col};
}
__device__ __forceinline__ TiledEdgeQueue tiled_edge_for(const TiledEdgeAtFlush &at, const TiledEdge &e) {
    return TiledEdgeQueue{e.values, e.n_values, at.slots};
}

// the decoder's: entry `cnt` of the queue gets the slot of bit `b`, the k-th set bit of the decoded word
__device__ __forceinline__ void tiled_edge_queue(int, int, int) {}
template <class P0, class... P>
__device__ __forceinline__ void tiled_edge_queue(int cnt, int b, int k, const P0 &p0, const P &...p) {
    if constexpr (std::is_same<P0, TiledEdgeRow>::value || std::is_same<P0, TiledEdgeCol>::value) p0.slots[cnt] = p0.slot(b, k);
    else tiled_edge_queue(cnt, b, k, p...);
}
// the adder's: the value of queue entry i
__device__ __forceinline__ float tiled_edge_value(int) { return 1.0f; }
template <class P0, class... P>
__device__ __forceinline__ float tiled_edge_value(int i, const P0 &p0, const P &...p) {
    if constexpr (tiled_is_edge<P0>::value && !std::is_same<P0, TiledEdge>::value) return p0.value(i);
    else return tiled_edge_value(i, p...);
}

// the refusals every entry with edge values adds to its own, in the order invalid, alignment, size
inline int tiled_edge_index_ok(const int64_t *val_ptr, const int16_t *val_row, int64_t n_tiles, size_t n_values) {
    if ((n_tiles > 0 && (!val_ptr || !val_row)) || n_values > static_cast<size_t>(INT32_MAX)) return QGTC_EINVAL;
    if ((reinterpret_cast<uintptr_t>(val_ptr) & 7u) || (reinterpret_cast<uintptr_t>(val_row) & 1u)) return QGTC_EALIGN;
    return QGTC_OK;
}
// two lists of refusals as one, in the entries' order: invalid before alignment before size
inline int tiled_edge_rc(int a, int b) {
    for (const int rc : {QGTC_EINVAL, QGTC_EALIGN, QGTC_ESIZE})
        if (a == rc || b == rc) return rc;
    return QGTC_OK;
}

}  // namespace
