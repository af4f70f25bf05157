"""Exact NumPy model of the scaled tiled products and the degrees (include/qgtc.h, "Scaled tiled products and degrees";
QGTC.tiledMM2Bit / tiledMM2Int with row_scale, TiledAdjacency.degrees / mean_scale), on top of tests/tiled_model.py:
y = fl32(fl32(sum) * row_scale[row]), one float32 multiply, and the expected words from the C oracle's value quantiser. No GPU."""
import numpy as np

from tiled_model import set_cells


def degrees(src, dst, n):
    """(out_deg, in_deg) int32 [n]: the set cells of every row and of every column of the quantised adjacency."""
    cells = set_cells(src, dst, n)
    return (np.bincount(cells // n, minlength=n).astype(np.int32), np.bincount(cells % n, minlength=n).astype(np.int32))


def mean_scale(deg):
    """1 / deg in float32 (one correctly rounded division), 0 where the degree is 0."""
    deg = np.asarray(deg)
    with np.errstate(divide="ignore"):
        inv = np.float32(1) / deg.astype(np.float32)
    return np.where(deg == 0, np.float32(0), inv).astype(np.float32)


def scaled(C, scale):
    """y [n, N] float32: the exact sums converted to float32 (round to nearest even), times the row's scale in float32."""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        y = np.asarray(C).astype(np.float32) * np.asarray(scale, dtype=np.float32)[:, None]
    assert y.dtype == np.float32
    return y


def expected_bits_scaled(oracle, y, ob):
    """The rows-layout words [ob][PAD8(n)][S128(N)*4] (flat uint32) of the value quantiser of y: what the scaled tiledMM2Bit gives."""
    return oracle.pack(oracle.quantize(y, ob), ob)
