"""Exact NumPy model of the edge values of the tiled adjacency (include/qgtc.h, "Edge values"; tiled.edge_slots / edge_endpoints /
edge_values, QGTC.tiledMMFloat(edge_weight=) on adj and adj.T, tiled.tiledSDDMM), on top of tests/tiled_model.py and
tests/tiled_float_model.py. The slot of a stored cell is its rank when the set bits are listed by tile id, then tile row, then column
ascending; the weighted fold adds fl32(values[slot] * X[v]) over a row's neighbours v in ascending id order, one np.float32 multiply
and one np.float32 add each; the SDDMM is DOT of tests/tiled_attn_model.py per stored cell. No GPU."""
import numpy as np

from tiled_attn_model import dot_f32 as DOT
from tiled_float_model import FLOAT_FORWARD_VARIANTS, FLOAT_TRANSPOSED_VARIANTS, float_variant
from tiled_model import np_tiled, set_cells

# The edge values end the pack of k_tiled_mm_f32 / k_tiled_mm_f32_t and the family launcher forwards the pack, so the weighted launch
# takes the shape its plain parent takes at every N (tiled_float_kernels.hip.h, tiled_row_width_switch / tiled_col_width_switch).
EDGE_FORWARD_VARIANTS = FLOAT_FORWARD_VARIANTS
EDGE_TRANSPOSED_VARIANTS = FLOAT_TRANSPOSED_VARIANTS
# k_tiled_sddmm keeps the row of A in registers up to N = 256 and reads it again per neighbour beyond (qgtc_tiled_sddmm.hip)
SDDMM_VARIANTS = ("registers", "reread")


def edge_variant(N, transposed):
    """The template variant the launcher picks at output width N."""
    return float_variant(N, transposed)


def sddmm_variant(N):
    return SDDMM_VARIANTS[0 if N <= 256 else 1]


def slot_cells(src, dst, n):
    """(row, col) int64 [nnz] of the stored cells in SLOT order: by 32-row block, then k-quad (that is tile id), then row, then column."""
    cells = set_cells(src, dst, n)
    r, c = cells // n, cells % n
    order = np.lexsort((c, r & 31, c >> 7, r >> 5))
    return r[order], c[order]


def value_index(src, dst, n):
    """(val_ptr int64 [T + 1], val_row int16 [T, 32]) from the model's tiles: the exclusive scan of the tiles' bit counts, and the set
    bits of each tile above each of its rows."""
    _, _, tiles = np_tiled(src, dst, n)
    T = tiles.shape[0]
    bits = np.unpackbits(np.ascontiguousarray(tiles).view(np.uint8).reshape(T, 32, 16), axis=2).sum(axis=2).astype(np.int64)   # [T, 32]
    per_row = bits.reshape(T, 32)
    val_row = (np.cumsum(per_row, axis=1) - per_row).astype(np.int16)
    val_ptr = np.concatenate([[0], np.cumsum(per_row.sum(axis=1))]).astype(np.int64)
    return val_ptr, val_row


def edge_slots(src, dst, n, s, d):
    """int64 [E]: the slot of cell (s[e], d[e]), -1 where it is not stored or an id is out of range."""
    r, c = slot_cells(src, dst, n)
    keys = r * n + c
    order = np.argsort(keys)
    s, d = np.asarray(s, dtype=np.int64), np.asarray(d, dtype=np.int64)
    ok = (s >= 0) & (s < n) & (d >= 0) & (d < n)
    want = np.where(ok, s * n + d, -1)
    pos = np.searchsorted(keys[order], want)
    pos = np.minimum(pos, max(keys.size - 1, 0))
    hit = ok & (keys.size > 0)
    if keys.size:
        hit &= keys[order][pos] == want
        return np.where(hit, order[pos], -1).astype(np.int64)
    return np.full(s.shape, -1, dtype=np.int64)


def _lists(src, dst, n, transposed):
    """(out_row, neighbour, slot) of the stored cells sorted by (output row, neighbour id) on the view, and every row's degree"""
    r, c = slot_cells(src, dst, n)
    slot = np.arange(r.size, dtype=np.int64)
    out_row, nb = (c, r) if transposed else (r, c)
    order = np.lexsort((nb, out_row))
    return out_row[order], nb[order], slot[order], np.bincount(out_row, minlength=n)


def weighted_f32(src, dst, n, X, values, transposed=False, scale=None):
    """float32 [n, N]: s = +0; s = fl32(s + fl32(values[slot_k] * X[v_k])) over the neighbours v_1 < v_2 < ... of each row of the view;
    times scale[row] if given."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    values = np.ascontiguousarray(values, dtype=np.float32)
    assert X.ndim == 2 and X.shape[0] == n
    out_row, nb, slot, deg = _lists(src, dst, n, transposed)
    assert values.shape == (slot.size,)
    start = np.concatenate([[0], np.cumsum(deg)[:-1]])
    out = np.zeros((n, X.shape[1]), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for k in range(int(deg.max()) if deg.size else 0):
            rows = np.flatnonzero(deg > k)
            pos = start[rows] + k
            term = values[slot[pos]][:, None] * X[nb[pos]]
            assert term.dtype == np.float32
            out[rows] = out[rows] + term
        if scale is not None:
            out = out * np.asarray(scale, dtype=np.float32)[:, None]
    assert out.dtype == np.float32
    return out


def sddmm_f32(src, dst, n, A, B, transposed=False):
    """float32 [nnz] in slot order: DOT(A[i], B[j]) for the stored cell (i, j); on the transposed view the cell (i, j) of the adjacency
    gets DOT(A[j], B[i]) (row j of the view's A, row i of its B)."""
    r, c = slot_cells(src, dst, n)
    A, B = np.ascontiguousarray(A, dtype=np.float32), np.ascontiguousarray(B, dtype=np.float32)
    if r.size == 0:
        return np.zeros(0, dtype=np.float32)
    return DOT(A[c], B[r]) if transposed else DOT(A[r], B[c])
