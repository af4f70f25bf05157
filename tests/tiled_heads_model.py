"""The exact models of the multi-head entries (include/qgtc_heads.h): each is the existing single-head model of
tests/tiled_edge_model.py / tests/tiled_esoftmax_model.py applied per head - to the column slice h d .. (h + 1) d - 1 of the node
matrices and to element [:, h] of the per-edge vectors. That IS the contract: a head's result is bit for bit the single-head call's
on its contiguous slice, so nothing is modelled twice. Per-edge vectors are float32 [nnz, H], head-minor; statistics are [n, H]."""
import numpy as np

import tiled_edge_model as em
import tiled_esoftmax_model as sm

F32 = np.float32

# the (heads, columns per head) every test of the heads uses: a head of one; two; a non-power-of-two d in 8-lane groups; 8 heads in one
# wave pass; 16- and 32-lane groups; d = 48 padded to a wave; three whole-wave heads; d > 64, a head on two slots; and two widths past
# the register path (H * 64 = 320 columns; a padded width of 40 * 8 = 320)
HEAD_SHAPES = ((1, 5), (2, 8), (3, 5), (8, 8), (4, 16), (2, 32), (2, 48), (3, 64), (2, 100), (5, 64), (40, 8))
# beyond them, for the per-edge dot alone: d > 64 on six register slots, and d > 64 past the register path
SDDMM_MORE_SHAPES = ((3, 80), (2, 200))


def head_cols(h, d):
    return slice(h * d, (h + 1) * d)


def sddmm_heads_f32(src, dst, n, A, B, heads, transposed=False):
    """float32 [nnz, H]: column h is em.sddmm_f32 on head h's columns of A and B"""
    A, B = np.ascontiguousarray(A, dtype=F32), np.ascontiguousarray(B, dtype=F32)
    assert A.shape == B.shape and A.shape[1] % heads == 0
    d = A.shape[1] // heads
    cols = [em.sddmm_f32(src, dst, n, A[:, head_cols(h, d)], B[:, head_cols(h, d)], transposed) for h in range(heads)]
    return np.ascontiguousarray(np.stack(cols, axis=1), dtype=F32)


def weighted_heads_f32(src, dst, n, X, values, transposed=False, scale=None):
    """float32 [n, N]: head h's columns are em.weighted_f32 of head h's columns of X with the weights values[:, h]"""
    X, values = np.ascontiguousarray(X, dtype=F32), np.ascontiguousarray(values, dtype=F32)
    heads = values.shape[1]
    assert X.shape[1] % heads == 0
    d = X.shape[1] // heads
    out = np.zeros_like(X)
    for h in range(heads):
        out[:, head_cols(h, d)] = em.weighted_f32(src, dst, n, X[:, head_cols(h, d)], values[:, h], transposed, scale)
    return out


def edge_softmax_heads_f32(src, dst, n, logits, transposed=False):
    """(alpha [nnz, H], m [n, H], inv [n, H]): column h is sm.edge_softmax_f32 of logits[:, h]"""
    logits = np.ascontiguousarray(logits, dtype=F32)
    parts = [sm.edge_softmax_f32(src, dst, n, logits[:, h], transposed) for h in range(logits.shape[1])]
    return tuple(np.ascontiguousarray(np.stack([p[i] for p in parts], axis=1), dtype=F32) for i in range(3))


def edge_softmax_grad_heads_f32(src, dst, n, alpha, g, transposed=False):
    """float32 [nnz, H]: column h is sm.edge_softmax_grad_f32 of alpha[:, h] and g[:, h]"""
    alpha, g = np.ascontiguousarray(alpha, dtype=F32), np.ascontiguousarray(g, dtype=F32)
    cols = [sm.edge_softmax_grad_f32(src, dst, n, alpha[:, h], g[:, h], transposed) for h in range(alpha.shape[1])]
    return np.ascontiguousarray(np.stack(cols, axis=1), dtype=F32)


def edge_attention_heads_f32(src, dst, n, Q, K, V, heads, scale=None, transposed=False):
    """float32 [n, N]: head h's columns are sm.edge_attention_f32 on head h's columns of Q, K and V; scale defaults to 1 / sqrt(d)"""
    Q, K, V = (np.ascontiguousarray(t, dtype=F32) for t in (Q, K, V))
    d, dv = Q.shape[1] // heads, V.shape[1] // heads
    scale = 1.0 / np.sqrt(d) if scale is None else scale
    out = np.zeros_like(V)
    for h in range(heads):
        out[:, head_cols(h, dv)] = sm.edge_attention_f32(src, dst, n, Q[:, head_cols(h, d)], K[:, head_cols(h, d)], V[:, head_cols(h, dv)],
                                                         scale, transposed)[0]
    return out


def edge_attention_grads_heads_f32(src, dst, n, Q, K, V, heads, dY, scale=None, transposed=False):
    """(dQ, dK, dV): per head sm.edge_attention_grads_f32 on the head's columns"""
    Q, K, V, dY = (np.ascontiguousarray(t, dtype=F32) for t in (Q, K, V, dY))
    d, dv = Q.shape[1] // heads, V.shape[1] // heads
    scale = 1.0 / np.sqrt(d) if scale is None else scale
    dQ, dK, dV = np.zeros_like(Q), np.zeros_like(K), np.zeros_like(V)
    for h in range(heads):
        c, cv = head_cols(h, d), head_cols(h, dv)
        dQ[:, c], dK[:, c], dV[:, cv] = sm.edge_attention_grads_f32(src, dst, n, Q[:, c], K[:, c], V[:, cv], scale, dY[:, cv], transposed)
    return dQ, dK, dV


def sddmm_heads_variant(N, heads):
    """(the lane mapping, register slots) qgtc_tiled_sddmm_heads_f32 takes for N columns in `heads` heads: "narrow" - a head on an
    aligned group of P = next_pow2(d) lanes, ceil(H P / 64) slots - or "wide" - a head on the whole wave, H ceil(d / 64) slots -; 0
    slots is the re-reading path."""
    d = N // heads
    if d > 64:
        need = heads * ((d + 63) // 64) if N <= 256 else 7
        return "wide", 4 if need <= 4 else 6 if need <= 6 else 0
    P = 1
    while P < d:
        P *= 2
    need = (heads * P + 63) // 64
    return "narrow", 1 if need <= 1 else 2 if need <= 2 else 4 if need <= 4 else 0
