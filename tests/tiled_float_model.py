"""Exact NumPy model of the float tiled products (include/qgtc.h, "Float tiled products"; QGTC.tiledMMFloat on adj and adj.T), on top
of tests/tiled_model.py: every output row adds the float32 rows of X of its neighbours in ASCENDING id order, starting from +0, one
np.float32 add each, then (with a scale) one np.float32 multiply. The order is the contract, so the result is compared with the
device's bit for bit. No GPU."""
import numpy as np

from tiled_model import set_cells

# (lanes per output row, columns per lane) of k_tiled_mm_f32 by output width N (tiled_float_kernels.hip.h, tiled_row_width_switch:
# 16 / 32 / 64 / 128 columns a workgroup up to those N, 256-column chunks beyond), and of k_tiled_mm_f32_t (the same header,
# tiled_col_width_switch: 16 / 32 columns a workgroup up to those N, 64-column chunks beyond). Every pack - plain, source scale,
# edge dropout, node masks - goes through that one switch.
FLOAT_FORWARD_VARIANTS = ((16, 1), (16, 2), (16, 4), (32, 4), (64, 4))
FLOAT_TRANSPOSED_VARIANTS = ((16, 1), (16, 2), (16, 4))


def float_variant(N, transposed):
    """The template variant the launcher picks at output width N."""
    if transposed:
        return FLOAT_TRANSPOSED_VARIANTS[0 if N <= 16 else 1 if N <= 32 else 2]
    return FLOAT_FORWARD_VARIANTS[0 if N <= 16 else 1 if N <= 32 else 2 if N <= 64 else 3 if N <= 128 else 4]


def float_chunks(N, transposed):
    """Workgroups along the output width (grid.y)."""
    lpr, cpl = float_variant(N, transposed)
    width = lpr * cpl
    return (N + width - 1) // width


def neighbour_lists(src, dst, n, transposed=False):
    """(out_row, neighbour) int64 arrays of the set cells sorted by (output row, neighbour id), and the degree of every row."""
    cells = set_cells(src, dst, n)
    r, c = cells // n, cells % n
    out_row, nb = (c, r) if transposed else (r, c)
    order = np.lexsort((nb, out_row))
    out_row, nb = out_row[order], nb[order]
    return out_row, nb, np.bincount(out_row, minlength=n)


def aggregate_f32(src, dst, n, X, transposed=False, scale=None, descending=False):
    """float32 [n, N]: s = +0; s = fl32(s + X[v_k]) over the neighbours v_1 < v_2 < ... of each row; times scale[row] if given.
    The k-th neighbour's row is added for all rows at once, k = 0 .. max degree - 1. `descending` adds in the opposite order (a test
    aid: it shows that the order matters on given inputs)."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    assert X.ndim == 2 and X.shape[0] == n
    out_row, nb, deg = neighbour_lists(src, dst, n, transposed)
    start = np.concatenate([[0], np.cumsum(deg)[:-1]])
    out = np.zeros((n, X.shape[1]), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for k in range(int(deg.max()) if deg.size else 0):
            rows = np.flatnonzero(deg > k)
            pos = start[rows] + (deg[rows] - 1 - k if descending else k)
            out[rows] = out[rows] + X[nb[pos]]
        if scale is not None:
            out = out * np.asarray(scale, dtype=np.float32)[:, None]
    assert out.dtype == np.float32
    return out
