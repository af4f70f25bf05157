// tiled_bit_nodes.hip.h — part of libqgtc_hip.so (included by qgtc_tiled_bit_nodes.hip and qgtc_tiled_bit_t_nodes.hip): what the four
// masked bit products of include/qgtc_bitnodes.h do, on either view - the checks of the _scaled twin (without its refusal of a NULL
// row_scale: here NULL is the plain sum), then those of the node masks, then the launch with the pack (TiledNodes) or
// (row_scale, TiledNodes). All of it runs before any device work. It needs the view's kernel header before it.
#pragma once

#include "tiled_args.hip.h"
#include "tiled_nodes.hip.h"

namespace {

template <int MODE, class Index>
int tiled_mm_nodes_entry(const Index &ix, const uint32_t *tiles, int64_t n_tiles, int n, const uint32_t *X, size_t x_words, int N, int bit2,
                         int output_bit, const float *row_scale, void *out, size_t out_size, const uint32_t *row_mask,
                         const uint32_t *nbr_mask, size_t mask_words, void *stream) {
    int rc = tiled_mm_args_ok(ix, tiles, n_tiles, n, X, N, bit2, out);
    if (rc != QGTC_OK) return rc;
    if (MODE == 0 && !bits_ok(output_bit)) return QGTC_EINVAL;
    if (out_size < (MODE == 0 ? qgtc_rows_words(n, N, output_bit) : static_cast<size_t>(n) * N)) return QGTC_ESIZE;
    rc = tiled_nodes_args_ok(row_mask, nbr_mask, mask_words, n);
    if (rc != QGTC_OK) return rc;
    const TiledNodes nodes{row_mask, nbr_mask};
    const hipStream_t st = static_cast<hipStream_t>(stream);
    return row_scale ? tiled_mm_launch<MODE>(ix, tiles, n_tiles, n, X, x_words, N, bit2, output_bit, out, st, row_scale, nodes)
                     : tiled_mm_launch<MODE>(ix, tiles, n_tiles, n, X, x_words, N, bit2, output_bit, out, st, nodes);
}

}  // namespace
