"""The byte-code route of affine quantisation (include/qgtc_codes.h, qgtc_ppopp22_amd/affine.py), bit for bit, in
NumPy, on top of tests/affine_model.py (nothing of it is restated): the codes as bytes, their exact neighbour sums on a view's matrix under
node masks, and the fused aggregate - ``am.dequant`` on those sums with the masked degrees. Shared by the CPU tests of the model and the
GPU tests. No GPU."""
import numpy as np

import affine_model as am


def pad4(W):
    return (W + 3) // 4 * 4


def codes(x, qp, bits):
    """uint8 [H, W]: the codes of ``am.quantise``, one byte each."""
    q = am.quantise(x, qp, bits)
    assert int(q.min(initial=0)) >= 0 and int(q.max(initial=0)) <= 255
    return q.astype(np.uint8)


def codes_buffer(x, qp, bits, ld=None, fill=0):
    """uint8 [H, ld] as qgtc_affine_codes leaves a buffer that held ``fill``: the codes, zeros up to PAD4(W), ``fill`` beyond."""
    q = codes(x, qp, bits)
    H, W = q.shape
    ld = pad4(W) if ld is None else ld
    buf = np.full((H, ld), fill, dtype=np.uint8)
    buf[:, :pad4(W)] = 0
    buf[:, :W] = q
    return buf


def sums(A, Q, row_mask=None, nbr_mask=None):
    """int64 [n, N]: the exact sum of the code rows over the live neighbours of every row of the view's matrix A."""
    return am.masked_view(A, row_mask, nbr_mask) @ np.asarray(Q, dtype=np.int64)


def tiled_mm_codes(A, Q, row_mask=None, nbr_mask=None):
    """int32 [n, N] of affine.tiledMMCodes."""
    acc = sums(A, Q, row_mask, nbr_mask)
    assert int(acc.max(initial=0)) < 2 ** 31
    return acc.astype(np.int32)


def fused(A, Q, qt, row_scale=None, row_mask=None, nbr_mask=None):
    """float32 [n, N] of the _affine entries: ``am.dequant`` of the sums with the identity on the left, the masked degrees as the row sums
    and ``qt`` ([1, 4]) on the right."""
    Am = am.masked_view(A, row_mask, nbr_mask)
    acc = sums(A, Q, row_mask, nbr_mask)
    assert int(acc.max(initial=0)) < 2 ** 24, "am.dequant takes the sums as float32"
    return am.dequant(acc.astype(np.float32), A.shape[0], am.IDENTITY, Am.sum(axis=1), qt, None, row_scale)


def aggregate(A, T, bits, row_scale=None, row_mask=None, nbr_mask=None):
    """float32 [n, N] of affine.aggregate(route="bytes"): qparams, codes, the fused entry."""
    T = np.ascontiguousarray(T, dtype=np.float32)
    qt = am.qparams(T, bits)
    return fused(A, codes(T, qt, bits), qt, row_scale, row_mask, nbr_mask)
