"""Exact NumPy model of the attention tiled products with HEADS (include/qgtc_attn_heads.h; QGTC.tiledMMFloat(attn=) and
QGTC.tiledAggregate(attn=) with scores [n, H]): tests/tiled_attn_model.py applied per head - columns h d .. (h + 1) d - 1 of the node
matrices as an [n, d] matrix, element [:, h] of the [n, H] vectors as an [n] vector. Nothing is specified again, so the results are
compared with the device's bit for bit. Beside it, a hand-kept copy of the launchers' choices (tiled_attn_heads_kernels.hip.h,
tiled_attn_heads_t_kernels.hip.h). No GPU."""
import numpy as np

from tiled_attn_model import ATT_TRANSPOSED_VARIANTS, att_variant, attention_f32, attention_grads_f32, dot_f32
from tiled_max_model import MAX, extremum_f32

F32 = np.float32

# the (H, d) of the device tests: d = 1; a d that is no power of two; the canonical 8 x 8 and 4 x 16; d just past 32; just past 64 (two
# slots a head); 85 (H d = 255 stays under 256); 129 (three slots a head)
HEAD_SHAPES = ((2, 1), (3, 5), (8, 8), (4, 16), (2, 33), (2, 65), (3, 85), (2, 129))
# past the issue's list: two columns a lane, narrow heads on four and on six slots (blockIdx.y), and a head wider than 256, which is
# read again
MORE_SHAPES = ((3, 8), (8, 32), (12, 32), (2, 257))

PRODUCT_VARIANTS = ATT_TRANSPOSED_VARIANTS      # 16 lanes a row on either view: (16, 1), (16, 2), (16, 4)
GRAD_VARIANTS = (("narrow", 1), ("wide", 4), ("wide", 0))


def product_variant(H, d, transposed):
    """(lanes per output row, columns per lane) of the product launcher: the column view's table at N = H d on either view (at most 64
    columns a workgroup); on the column view the chunk is narrowed until a lane's columns fit in one head's d."""
    N = H * d
    if transposed:
        N = N if d >= 4 else (min(N, 32) if d >= 2 else 16)
    return att_variant(N, True)


def product_chunks(H, d, transposed):
    lpr, cpl = product_variant(H, d, transposed)
    return (H * d + lpr * cpl - 1) // (lpr * cpl)


def lanes_straddle_heads(H, d, transposed):
    """Whether some lane's CPL adjacent columns belong to two heads (the lane then computes two weights a neighbour)."""
    cpl = product_variant(H, d, transposed)[1]
    return H > 1 and d % cpl != 0


def grad_variant(H, d):
    """((mapping, register slots), blockIdx.y extent) of the score gradient: tiled_atth_shape."""
    if d > 64:
        return ("wide", 4 if d <= 256 else 0), H
    P = 1
    while P < d:
        P *= 2
    return ("narrow", 1), (H * P + 63) // 64


def _slice(t, h, d):
    return np.ascontiguousarray(t[:, h * d:(h + 1) * d])


def _heads(X, att_out):
    X, p = np.asarray(X), np.asarray(att_out)
    assert X.ndim == 2 and p.ndim == 2 and p.shape[0] == X.shape[0] and X.shape[1] % p.shape[1] == 0
    return p.shape[1], X.shape[1] // p.shape[1]


def max_heads_f32(src, dst, n, att_nbr, transposed=False):
    """M float32 [n, H]: the largest att_nbr[k, h] over each row's neighbours - the maximum is exact and independent per column."""
    return extremum_f32(src, dst, n, np.ascontiguousarray(att_nbr, dtype=F32), transposed, MAX)[0]


def attention_heads_f32(src, dst, n, X, att_out, att_nbr, slope=0.2, transposed=False, wrong=None):
    """(out float32 [n, H d], m float32 [n, H], inv float32 [n, H]). `wrong` = "next_head" is a WRONG rule, a test aid: head h reads
    head h + 1's scores (the last one head 0's)."""
    assert wrong in (None, "next_head")
    H, d = _heads(X, att_out)
    p, q = np.ascontiguousarray(att_out, dtype=F32), np.ascontiguousarray(att_nbr, dtype=F32)
    out, m, inv = np.empty((n, H * d), F32), np.empty((n, H), F32), np.empty((n, H), F32)
    for h in range(H):
        s = (h + 1) % H if wrong == "next_head" else h
        out[:, h * d:(h + 1) * d], m[:, h], inv[:, h] = attention_f32(src, dst, n, _slice(X, h, d), p[:, s].copy(), q[:, s].copy(), slope,
                                                                     transposed)
    return out, m, inv


def attention_grads_heads_f32(src, dst, n, X, att_out, att_nbr, dY, Y, m, inv, slope=0.2, transposed=False, wrong=None):
    """(dX [n, H d], dp [n, H], dq [n, H], D [n, H]) of the backward of attention_heads_f32 from its Y, m and inv."""
    assert wrong in (None, "next_head")
    H, d = _heads(X, att_out)
    p, q = np.ascontiguousarray(att_out, dtype=F32), np.ascontiguousarray(att_nbr, dtype=F32)
    dX, dp, dq, D = np.empty((n, H * d), F32), np.empty((n, H), F32), np.empty((n, H), F32), np.empty((n, H), F32)
    for h in range(H):
        s = (h + 1) % H if wrong == "next_head" else h
        dX[:, h * d:(h + 1) * d], dp[:, h], dq[:, h], D[:, h] = attention_grads_f32(
            src, dst, n, _slice(X, h, d), p[:, s].copy(), q[:, s].copy(), _slice(dY, h, d), _slice(Y, h, d), m[:, h].copy(), inv[:, h].copy(),
            slope, transposed)
    return dX, dp, dq, D


def rowdot_heads_f32(A, B, H):
    d = A.shape[1] // H
    return np.stack([dot_f32(_slice(A, h, d), _slice(B, h, d)) for h in range(H)], axis=1) if A.shape[0] else np.zeros((0, H), F32)
