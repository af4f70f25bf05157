// tiled_nodes.hip.h — part of libqgtc_hip.so (included by tiled_float_kernels.hip.h): node masks on the tile walk (include/qgtc.h,
// "Node masks"). A node set is a bitmap in the bit order of a tile row (node i at word i >> 5, bit
// 31 - (i & 31)), S128(n) * 4 words, so the four words that belong to a tile's 128 columns are one aligned 16-byte read and restricting
// the neighbours is an AND of a tile word with a bitmap word before the MSB-first decode: a neighbour outside the set is never queued.
// Restricting the output rows is decided from blockIdx-indexed words: a dead workgroup reads no index and no tile.
//
// The kernels take the masks as the LAST element of their trailing template pack (TiledNodes), like the edge-dropout mask: no such
// element, and every `if constexpr` below is discarded and the kernels are the ones that existed. Either pointer may be null, which
// means all nodes: one uniform select per word read, not a second set of instantiations (DESIGN.md section 6.15e has the counts).
#pragma once

#include <cstdint>
#include <type_traits>

#include "tiled_drop.hip.h"

namespace {

struct TiledNodes {
    const uint32_t *row;   // the output rows that are computed, or null: all
    const uint32_t *nbr;   // the neighbours that take part, or null: all
    // the pack's per-neighbour question (tiled_drop_kept): the bitmap has been ANDed into the decode word already
    __device__ __forceinline__ bool kept(int) const { return true; }
};

// a mask element of the pack: no operand of the product
template <>
struct tiled_is_drop<TiledNodes> { static constexpr bool value = true; };

template <class... P>
constexpr bool tiled_has_nodes() { return (false || ... || std::is_same<P, TiledNodes>::value); }

__device__ __forceinline__ TiledNodes tiled_nodes_of() { return TiledNodes{nullptr, nullptr}; }
template <class P0, class... P>
__device__ __forceinline__ TiledNodes tiled_nodes_of(const P0 &p0, const P &...p) {
    if constexpr (std::is_same<P0, TiledNodes>::value) return p0;
    else return tiled_nodes_of(p...);
}

// word `i` of a bitmap, all ones without one. `i` must be the same for every lane of the wave: the index is made provably uniform so
// that the read is a scalar load.
__device__ __forceinline__ uint32_t tiled_nodes_word(const uint32_t *__restrict__ bm, int i) {
    return bm ? bm[__builtin_amdgcn_readfirstlane(i)] : 0xffffffffu;
}
// the four words of k-quad `q` (16-byte aligned by contract), under the same condition
__device__ __forceinline__ uint4 tiled_nodes_quad(const uint32_t *__restrict__ bm, int q) {
    return bm ? *reinterpret_cast<const uint4 *>(bm + __builtin_amdgcn_readfirstlane(q) * 4) : make_uint4(~0u, ~0u, ~0u, ~0u);
}
// whether element `i` (0 .. 31) of a bitmap word is set
__device__ __forceinline__ bool tiled_nodes_bit(uint32_t word, int i) { return (word >> (31 - i)) & 1u; }

// What the row-view kernels keep for the masks while they walk a block's tiles. Without masks the struct is empty and every question is
// answered by a constant, so the kernels' code is what it was.
template <bool NODES>
struct TiledNodesWalk {
    __device__ __forceinline__ static constexpr bool block_live() { return true; }
    __device__ __forceinline__ static constexpr bool row_live() { return true; }
    __device__ __forceinline__ static constexpr bool tile_live() { return true; }
    __device__ __forceinline__ static constexpr uint32_t word(int) { return 0xffffffffu; }
};
template <>
struct TiledNodesWalk<true> {
    TiledNodes nodes;
    uint32_t rword;   // the row bitmap's word of this 32-row block
    bool mine;        // this lane's tile row (lane l < RPG: row g * RPG + l) belongs to a row of the row bitmap
    uint4 nb, nbn;    // the neighbour bitmap's words of this tile's k-quad and of the next tile's
    __device__ __forceinline__ void start(const TiledNodes &nd, int rb, int my_row) {
        nodes = nd;
        rword = tiled_nodes_word(nodes.row, rb);
        mine = tiled_nodes_bit(rword, my_row & 31);
        nb = nbn = make_uint4(0, 0, 0, 0);
    }
    __device__ __forceinline__ void load(uint4 &to, int q, int nq) const {
        if (static_cast<unsigned>(q) < static_cast<unsigned>(nq)) to = tiled_nodes_quad(nodes.nbr, q);
    }
    __device__ __forceinline__ bool block_live() const { return rword != 0; }
    __device__ __forceinline__ bool row_live() const { return mine; }
    __device__ __forceinline__ bool tile_live() const { return (nb.x | nb.y | nb.z | nb.w) != 0; }
    __device__ __forceinline__ uint32_t word(int k) const { return k == 0 ? nb.x : k == 1 ? nb.y : k == 2 ? nb.z : nb.w; }
};
// `base` alone without masks, `base && live` with them
template <bool NODES>
__device__ __forceinline__ bool tiled_nodes_and(bool base, bool live) {
    if constexpr (NODES) return base && live;
    else return base;
}

// the refusals of the _nodes entries, made before any device work
inline int tiled_nodes_args_ok(const uint32_t *row_mask, const uint32_t *nbr_mask, size_t mask_words, int n) {
    if ((row_mask || nbr_mask) && mask_words < static_cast<size_t>(step128(n)) * 4) return QGTC_ESIZE;
    if (!aligned16(row_mask) || !aligned16(nbr_mask)) return QGTC_EALIGN;
    return QGTC_OK;
}

}  // namespace
