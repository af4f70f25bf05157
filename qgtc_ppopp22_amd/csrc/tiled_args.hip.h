// tiled_args.hip.h — part of libqgtc_hip.so (included by tiled_kernels.hip.h, tiled_t_kernels.hip.h and tiled_float_kernels.hip.h, and
// through them by every unit of the tiled adjacency; by qgtc_reorder.hip for the grid rule): what the tiled units share on the host -
// the limit on n, the two views' index structs, the graph part of an argument check, the 1-D grid rule and the check and entry body of
// the bit products. All of it runs before any device work. It needs common.hip.h before it.
#pragma once

#include <cmath>
#include <type_traits>

namespace {

constexpr int TILED_MAX_N = 1 << 23;

// The two views' index arrays. The launchers of the two views are overloads on these structs, and the templates above them are written
// once for both views.
struct TiledRowIndex {
    const int64_t *row_ptr;
    const int32_t *kquad;
    bool ok() const { return row_ptr && kquad; }   // the `index_ok` of the argument checks
    bool ptr_ok() const { return row_ptr; }        // the array the bit kernels read even without tiles
};
struct TiledColIndex {
    const int64_t *col_ptr, *col_tile;
    const int32_t *col_rb;
    bool ok() const { return col_ptr && col_tile && col_rb; }
    bool ptr_ok() const { return col_ptr; }
};

template <int V>
using tiled_int = std::integral_constant<int, V>;

// The graph part of an argument check, as two predicates: every check reports all its QGTC_EINVAL causes, these among them, before any
// QGTC_EALIGN. `index_ok`: every index array of the view is there (they and `tiles` may be NULL only when n_tiles is 0).
inline bool tiled_adj_malformed(bool index_ok, const uint32_t *tiles, int64_t n_tiles, int n) {
    return n < 1 || n > TILED_MAX_N || n_tiles < 0 || (n_tiles && (!index_ok || !tiles));
}
inline bool tiled_adj_misaligned(const uint32_t *tiles) { return tiles && !aligned16(tiles); }

// blocks of 256 threads for a grid-stride loop over `items`: at least one, 8192 at the most
inline int tiled_grid_1d(uint64_t items) {
    const uint64_t b = (items + 255) / 256;
    return static_cast<int>(b < 8192 ? (b ? b : 1) : 8192);
}

// ---- the bit products (qgtc_tiledmm2bit / 2int, their _t, _scaled and _t_scaled twins) ---------------------------------------------------
// The bit kernels read row_ptr / col_ptr without looking at n_tiles (the float kernels do not), so that array is wanted even when there
// are no tiles.
template <class Index>
inline int tiled_mm_args_ok(const Index &ix, const uint32_t *tiles, int64_t n_tiles, int n, const uint32_t *X, int N, int bit2,
                            const void *out) {
    if (!ix.ptr_ok() || !X || !out || N < 1 || bit2 < 1 || bit2 > 8 || tiled_adj_malformed(ix.ok(), tiles, n_tiles, n))
        return QGTC_EINVAL;
    if (!aligned16(X) || !aligned16(out) || tiled_adj_misaligned(tiles)) return QGTC_EALIGN;
    return QGTC_OK;
}

// 2^ob and 2^ob - 1 as floats: what the bit kernels' requantiser clamps to for ob output bits
struct TiledClamp {
    float maxv, maxm1;
    explicit TiledClamp(int ob) : maxv(std::ldexp(1.0f, ob)), maxm1(maxv - 1.0f) {}
};

// The launchers of the two kernels, at the foot of tiled_kernels.hip.h and tiled_t_kernels.hip.h: `scale` is () or (row_scale), and
// either with the node masks (a TiledNodes of tiled_nodes.hip.h) behind it.
template <int MODE, class... Scale>
int tiled_mm_launch(const TiledRowIndex &ix, const uint32_t *tiles, int64_t n_tiles, int n, const uint32_t *X, size_t x_words, int N,
                    int bit2, int ob, void *out, hipStream_t st, Scale... scale);
template <int MODE, class... Scale>
int tiled_mm_launch(const TiledColIndex &ix, const uint32_t *tiles, int64_t n_tiles, int n, const uint32_t *X, size_t x_words, int N,
                    int bit2, int ob, void *out, hipStream_t st, Scale... scale);

// What the eight entries do, on either view: the shared check, the entry's own arguments (a row_scale in the pack must be there;
// output_bit for MODE 0, the bit output), the output's size, the launch. MODE 2 (float32 [n, N]) is given output_bit = 1. A unit
// instantiates the kernels of the view and the pack it passes and no others.
template <int MODE, class Index, class... Scale>
int tiled_mm_entry(const Index &ix, const uint32_t *tiles, int64_t n_tiles, int n, const uint32_t *X, size_t x_words, int N, int bit2,
                   int output_bit, void *out, size_t out_size, void *stream, Scale... scale) {
    const int rc = tiled_mm_args_ok(ix, tiles, n_tiles, n, X, N, bit2, out);
    if (rc != QGTC_OK) return rc;
    if ((... || !scale) || (MODE == 0 && !bits_ok(output_bit))) return QGTC_EINVAL;
    if (out_size < (MODE == 0 ? qgtc_rows_words(n, N, output_bit) : static_cast<size_t>(n) * N)) return QGTC_ESIZE;
    return tiled_mm_launch<MODE>(ix, tiles, n_tiles, n, X, x_words, N, bit2, output_bit, out, static_cast<hipStream_t>(stream), scale...);
}

}  // namespace
