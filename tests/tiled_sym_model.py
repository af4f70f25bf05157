"""Exact NumPy model of the float tiled products with a source scale (include/qgtc.h, "Source scale"; QGTC.tiledMMFloat(adj, X,
row_scale, src_scale), QGTC.tiledAggregate and its backward), on top of tests/tiled_float_model.py: every output row adds
fl32(src_scale[v] * X[v]) over its neighbours v in ascending id order - one np.float32 multiply, then one np.float32 add, never fused -
then (with a row scale) one np.float32 multiply. Plus the inverse square roots of the degrees (TiledAdjacency.sym_scale) and the
edge-list preparation QGTC.add_self_loops. No GPU."""
import numpy as np

from tiled_float_model import neighbour_lists


def aggregate_f32_src(src, dst, n, X, transposed=False, scale=None, src_scale=None, fused=False, by_output_row=False):
    """float32 [n, N]: s = +0; s = fl32(s + fl32(src_scale[v_k] * X[v_k])) over the neighbours v_1 < v_2 < ... of each row; times
    scale[row] if given. With src_scale None it is tiled_float_model.aggregate_f32. Test aids, each a WRONG kernel: `fused` forms
    every term and add as one fma (exactly: float32 products and sums are exact in float64, one rounding to float32);
    `by_output_row` takes the factor of the output row in place of the neighbour's."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    assert X.ndim == 2 and X.shape[0] == n
    c = None if src_scale is None else np.ascontiguousarray(src_scale, dtype=np.float32)
    assert c is None or c.shape == (n,)
    out_row, nb, deg = neighbour_lists(src, dst, n, transposed)
    start = np.concatenate([[0], np.cumsum(deg)[:-1]])
    out = np.zeros((n, X.shape[1]), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for k in range(int(deg.max()) if deg.size else 0):
            rows = np.flatnonzero(deg > k)
            v = nb[start[rows] + k]
            if c is None:
                out[rows] = out[rows] + X[v]
            elif fused:
                # a float32 product has at most 48 significant bits and fits a float64; adding a float32 to it may round in float64
                # before the final rounding (double rounding), which only makes this emulation differ from a true fma in rare ties
                out[rows] = (out[rows].astype(np.float64) + c[rows if by_output_row else v].astype(np.float64)[:, None]
                             * X[v].astype(np.float64)).astype(np.float32)
            else:
                term = c[rows if by_output_row else v][:, None] * X[v]
                assert term.dtype == np.float32
                out[rows] = out[rows] + term
        if scale is not None:
            out = out * np.asarray(scale, dtype=np.float32)[:, None]
    assert out.dtype == np.float32
    return out


def inv_sqrt_degree(deg):
    """float32 [n]: np.float32(1) / np.sqrt(np.float32(deg)), both correctly rounded (IEEE), 0 where the degree is 0."""
    d = np.asarray(deg).astype(np.float32)
    out = np.zeros(d.shape, dtype=np.float32)
    nz = d > 0
    out[nz] = np.float32(1) / np.sqrt(d[nz])
    assert out.dtype == np.float32
    return out


def add_self_loops(src, dst, n):
    """(src, dst) without the existing (i, i) edges and with one loop per node appended (QGTC.add_self_loops)."""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    keep = src != dst
    loops = np.arange(n, dtype=np.int64)
    return np.concatenate([src[keep], loops]), np.concatenate([dst[keep], loops])


def error_bound(src, dst, n, X, transposed, scale, src_scale):
    """(the float64 result r . sum c_v x_v, the bound (d + 2) 2^-24 |r| sum |c_v x_v|), both [n, N] float64: a term passes through at
    most d + 1 roundings on its way into the sum of a row of degree d (its own multiply and at most d adds - Higham's recursive
    summation with one more rounding per term), and the final multiply by r adds one."""
    X = np.asarray(X, dtype=np.float64)
    c = np.ones(n) if src_scale is None else np.asarray(src_scale, dtype=np.float64)
    r = np.ones(n) if scale is None else np.asarray(scale, dtype=np.float64)
    out_row, nb, deg = neighbour_lists(src, dst, n, transposed)
    mag = np.zeros((n, X.shape[1]))
    np.add.at(mag, out_row, np.abs(c[nb][:, None] * X[nb]))
    exact = np.zeros((n, X.shape[1]))
    np.add.at(exact, out_row, c[nb][:, None] * X[nb])
    return exact * r[:, None], (deg[:, None] + 2) * 2.0 ** -24 * np.abs(r)[:, None] * mag
