// tiled_args.hip.h — part of libqgtc_hip.so (included by qgtc_tiled.hip, qgtc_tiled_t.hip and their scaled counterparts): the argument
// checks the tiled product entries share, made before any device work.
#pragma once

namespace {

constexpr int TILED_MAX_N = 1 << 23;

int tiled_mm_args_ok(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const uint32_t *X,
                     int N, int bit2, const void *out) {
    if (!row_ptr || !X || !out || n < 1 || n > TILED_MAX_N || N < 1 || bit2 < 1 || bit2 > 8 || n_tiles < 0 ||
        (n_tiles && (!kquad || !tiles)))
        return QGTC_EINVAL;
    if (!aligned16(X) || !aligned16(out) || (tiles && !aligned16(tiles))) return QGTC_EALIGN;
    return QGTC_OK;
}

int tiled_mm_t_args_ok(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles, int64_t n_tiles,
                       int n, const uint32_t *X, int N, int bit2, const void *out) {
    if (!col_ptr || !X || !out || n < 1 || n > TILED_MAX_N || N < 1 || bit2 < 1 || bit2 > 8 || n_tiles < 0 ||
        (n_tiles && (!col_tile || !col_rb || !tiles)))
        return QGTC_EINVAL;
    if (!aligned16(X) || !aligned16(out) || (tiles && !aligned16(tiles))) return QGTC_EALIGN;
    return QGTC_OK;
}

}  // namespace
