"""Exact NumPy model of fixed-fanout neighbour sampling on the tile-compressed adjacency (include/qgtc_fanout.h; ``fanout=`` of
QGTC.tiledMMFloat / QGTC.tiledAggregate): the per-node thresholds, by sorting, and a filter over the set cells of tests/tiled_model.py.
Masking is dropping, so the filtered edge list feeds the float, extremum and attention models unchanged. No GPU.

The hash H(i, j, seed) is tests/tiled_drop_model.py's, in A's coordinates on both axes. On ``axis`` "row" node u = i owns the cells of
row i, on "col" node u = j those of column j; thr[u] = 0 when u has at most k cells, otherwise the k-th largest of their hashes; a cell is
kept when H >= thr[u]."""
import numpy as np

from tiled_drop_model import H, SEEDS  # noqa: F401  (SEEDS: the seeds the GPU tests rotate)
from tiled_model import set_cells

AXES = ("row", "col")


def _cells(src, dst, n):
    cells = set_cells(src, dst, n)
    return cells // n, cells % n


def thresholds(src, dst, n, k, seed, axis):
    """uint32 [n]: thr of the rule above for the edge list's 1-bit adjacency (multiplicities quantised), by a sort of every node's hashes."""
    assert axis in AXES and k >= 1
    r, c = _cells(src, dst, n)
    h = H(r, c, seed).astype(np.int64)
    u = r if axis == "row" else c
    order = np.lexsort((-h, u))                    # by node, then by hash descending
    u_s, h_s = u[order], h[order]
    start = np.searchsorted(u_s, np.arange(n))
    deg = np.bincount(u, minlength=n)
    thr = np.zeros(n, dtype=np.uint32)
    big = np.nonzero(deg > k)[0]
    thr[big] = h_s[start[big] + k - 1].astype(np.uint32)
    return thr


def kept_mask(src, dst, n, k, seed, axis):
    """(rows, cols, keep): the set cells sorted by (row, column) and which of them the sample keeps."""
    r, c = _cells(src, dst, n)
    thr = thresholds(src, dst, n, k, seed, axis)
    return r, c, H(r, c, seed) >= thr[r if axis == "row" else c]


def kept_edges(src, dst, n, k, seed, axis):
    """(src, dst) int64: the set cells the sample keeps, each once, sorted by (row, column): an edge list of its own."""
    r, c, keep = kept_mask(src, dst, n, k, seed, axis)
    return r[keep], c[keep]
