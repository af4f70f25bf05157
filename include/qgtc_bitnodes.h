/* qgtc_bitnodes.h — node masks on the quantised tiled products of libqgtc_hip.so: requant(A . X) and its scaled
 * form on the subgraph INDUCED by two node sets, from the whole graph's tiles and without packing a second adjacency - a Cluster-GCN batch,
 * a last layer on the labelled nodes only, inference on a node subset. The terms view, k-quad, requant, quant1 and the layouts are those of
 * "Tile-compressed adjacency", "Transposed tiled adjacency" and "Scaled tiled products and degrees" in qgtc.h. The ABI version of qgtc.h
 * does not change: these are entries added beside it.
 *
 * A node set is the bitmap of "Node masks" in qgtc.h (qgtc_node_bitmap): uint32 words [S128(n) * 4], node i at word i >> 5, bit
 * 31 - (i & 31), 16-byte aligned, in the adjacency's numbering; bits from n up are never looked at. row_mask and nbr_mask are each a
 * bitmap or NULL (all nodes), relative to the view the ENTRY walks, as row_scale is: on the row view a row is A's row and a neighbour A's
 * column, on the column view (_t) the other way round. mask_words is the length of each bitmap given.
 *
 *   Output row o is computed iff o is in row_mask. Otherwise it holds exactly what a row without neighbours holds: the sum 0 through
 *   requant, or quant1(0.0f * row_scale[o]) when scaled, in the bit output; float 0, times row_scale[o] when scaled, in the float output.
 *   Neighbour k takes part iff k is in nbr_mask.
 *
 * The result is, word for word, the unmasked entry on qgtc_tiled_pack of the edges whose output-row end lies in row_mask and whose
 * neighbour end lies in nbr_mask. All-ones masks or two NULLs give the plain entry's words. Every word of out is written, as by the plain
 * entries: the rows of skipped blocks, the pad rows up to PAD8(n) and the columns past N (zeros) included.
 *
 * What is skipped. Row view (one workgroup per 32-row block rb and 128-column chunk): the block's rows are the one word row_mask[rb]; if it
 * is zero the workgroup reads neither row_ptr nor a tile nor X. Per tile of k-quad q the words nbr_mask[4q .. 4q + 3] are one 16-byte read;
 * if all four are zero the tile is skipped before X's planes are loaded. Column view (one workgroup per k-quad q and chunk, output rows
 * 128 q ..): the rows are row_mask[4q .. 4q + 3]; if all are zero the workgroup reads neither col_ptr nor a tile nor X. Per tile of row block
 * rb the neighbours are the one word nbr_mask[rb]; if it is zero the tile's X words are not loaded. So the tiles of a dead block and X's
 * words of dead neighbours may hold anything; index arrays must be valid throughout.
 *
 * row_scale is NULL for the plain sum (requant: the words of qgtc_tiledmm2bit / 2int and their _t on the induced edges); with a pointer it
 * is the value quantiser of the _scaled entries (float32 [n], y = float(sum) * row_scale[o], one IEEE single multiply).
 *
 * One launch on `stream`, no atomics on global memory, no host read; capturable. Refusals before any device work, in this order: those of
 * the _scaled twin (QGTC_EINVAL for a NULL X, out or view pointer, N < 1, bit2 outside 1 .. 8, a malformed adjacency and, for the bit
 * output, output_bit outside 1 .. 32; QGTC_EALIGN for X, out or tiles off a 16-byte boundary; QGTC_ESIZE for an out too small) - a NULL
 * row_scale is not one of them here -, then QGTC_ESIZE for mask_words < S128(n) * 4 when a mask is given, then QGTC_EALIGN for a mask off a
 * 16-byte boundary. */
#ifndef QGTC_BITNODES_H
#define QGTC_BITNODES_H

#include "qgtc.h"

#ifdef __cplusplus
extern "C" {
#endif

int qgtc_tiledmm2bit_nodes(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const uint32_t *X,
                           size_t x_words, int N, int bit2, int output_bit, const float *row_scale, uint32_t *out, size_t out_words,
                           const uint32_t *row_mask, const uint32_t *nbr_mask, size_t mask_words, void *stream);
int qgtc_tiledmm2int_nodes(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const uint32_t *X,
                           size_t x_words, int N, int bit2, const float *row_scale, float *out, size_t out_elems,
                           const uint32_t *row_mask, const uint32_t *nbr_mask, size_t mask_words, void *stream);
int qgtc_tiledmm2bit_t_nodes(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles, int64_t n_tiles,
                             int n, const uint32_t *X, size_t x_words, int N, int bit2, int output_bit, const float *row_scale,
                             uint32_t *out, size_t out_words, const uint32_t *row_mask, const uint32_t *nbr_mask, size_t mask_words,
                             void *stream);
int qgtc_tiledmm2int_t_nodes(const int64_t *col_ptr, const int64_t *col_tile, const int32_t *col_rb, const uint32_t *tiles, int64_t n_tiles,
                             int n, const uint32_t *X, size_t x_words, int N, int bit2, const float *row_scale, float *out,
                             size_t out_elems, const uint32_t *row_mask, const uint32_t *nbr_mask, size_t mask_words, void *stream);

#ifdef __cplusplus
}
#endif

#endif
