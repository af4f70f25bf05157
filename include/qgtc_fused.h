/* qgtc_fused.h — the middle of the static affine chain in one launch on libqgtc_hip.so: the re-quantising
 * walk qgtc_tiledmm_u8_requant and the chain product qgtc_affine_linear_chain (codes in) behind it, fused. In
 * agg(linear(agg(linear(X, W_in)), W_out)) this is the one pair that fuses without recomputation: the walk owns a 32-row block and ends
 * with that block's codes in registers, and the product reads exactly those rows. The codes cross LDS instead of memory. The adjacency,
 * the masks and the walk are those of qgtc_codes.h (row view only), the weight operand that of qgtc_linear.h, the code matrices, the
 * qparams rows and THE CODE OUTPUT those of qgtc_chain.h. The ABI version of qgtc.h does not change: this is an entry added beside it.
 *
 * THE CONTRACT: the result is, bit for bit, that of
 *   qgtc_tiledmm_u8_requant(row_ptr, kquad, tiles, n_tiles, n, Q, ld, q_bytes, K, t_qparams, agg_row_scale, h_qp, h_bits, H, ..,
 *                           row_mask, nbr_mask, mask_words, stream)                     H: a code matrix [n, K] under (h_qp, h_bits)
 *   qgtc_affine_linear_chain(NULL, H, .., n, K, h_qp, h_bits, codes_t, ldk, codes_bytes, N2, qb, groups_b, col_sums, lin_row_scale,
 *                            bias, relu, out, out_elems, outq, ldo, outq_bytes, out_qp, out_bits, stream)
 * with H never stored. A row outside row_mask, in a dead block or without live neighbours is float +0 after the walk, so the code zp of
 * h_qp, and goes through the product and its epilogue like any other: it takes lin_row_scale, bias and relu as the composed route's does.
 *
 * K is the hidden width (the walk's N, the product's K) and must fit one workgroup: K <= QGTC_FUSED_K_MAX. N2 <= QGTC_FUSED_N_MAX. The
 * column view (A^T) has no fused form; wider layers and that view take the two calls above.
 *
 * The entry makes one launch on `stream` (the last argument), uses no atomics, reads nothing back and allocates nothing: capturable.
 * Every output byte the entry owns is written: out [n, N2] whole, or of outq the bytes 0 .. PAD4(N2) - 1 of every row (cols .. PAD4 as
 * 0), bytes from PAD4(N2) on untouched. Refusals come before any device work, in this order: QGTC_EINVAL (a NULL required pointer, a
 * dimension < 1, K above QGTC_FUSED_K_MAX, N2 above QGTC_FUSED_N_MAX, a bit width outside 1 .. 8, groups other than 1 or N2, a
 * malformed adjacency, both outputs given or none), then QGTC_EALIGN (a code matrix or the weight codes off their rules; a qparams
 * table, tiles or a mask off a 16-byte boundary; a float32 or int32 buffer off a 4-byte boundary), then QGTC_ESIZE (a buffer too small;
 * mask_words < S128(n) * 4 when a mask is given). */
#ifndef QGTC_FUSED_H
#define QGTC_FUSED_H

#include "qgtc_chain.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QGTC_FUSED_K_MAX 256
#define QGTC_FUSED_N_MAX 256

/* Q, ld, q_bytes, K, t_qparams, agg_row_scale: the walk's code matrix [n, K], its row and the optional float32 [n] row scale of the
 * aggregate. h_qp, h_bits: the fixed per-tensor row the walk's result is re-quantised under (float32 [1][4], 16-byte aligned).
 * codes_t .. relu: as in qgtc_linear.h, with lin_row_scale float32 [n] or NULL. Exactly one of out (float32 [n, N2], contiguous,
 * out_elems >= n * N2) and outq (a code matrix [n, N2] with ldo, outq_bytes, under out_qp, out_bits); the other is NULL and its sizes
 * are ignored. row_mask, nbr_mask, mask_words: as in qgtc_codes.h. */
int qgtc_tiledmm_u8_linear(const int64_t *row_ptr, const int32_t *kquad, const uint32_t *tiles, int64_t n_tiles, int n, const uint8_t *Q,
                           size_t ld, size_t q_bytes, int K, const float *t_qparams, const float *agg_row_scale, const float *h_qp,
                           int h_bits, const uint8_t *codes_t, size_t ldk, size_t codes_bytes, int N2, const float *qb, int groups_b,
                           const int32_t *col_sums, const float *lin_row_scale, const float *bias, int relu, float *out, size_t out_elems,
                           uint8_t *outq, size_t ldo, size_t outq_bytes, const float *out_qp, int out_bits, const uint32_t *row_mask,
                           const uint32_t *nbr_mask, size_t mask_words, void *stream);

#ifdef __cplusplus
}
#endif

#endif
