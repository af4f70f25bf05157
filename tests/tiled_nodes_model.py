"""Exact NumPy model of node masks on the tile-compressed adjacency (include/qgtc.h, "Node masks"; ``row_mask=`` / ``nbr_mask=`` of
QGTC.tiledMMFloat / QGTC.tiledAggregate): the bitmap of a node set and a filter over the set cells of tests/tiled_model.py. Masking is
restricting the edge list, so the filtered list feeds the float, extremum and attention models unchanged (tests/tiled_float_model.py,
tiled_sym_model.py, tiled_max_model.py, tiled_attn_model.py). No GPU.

A node set is int32 words [S128(n) * 4], node i at word i >> 5, bit 31 - (i & 31); bits at positions >= n are zero. On a view the
output row o is computed iff o is in the row set R, and its neighbour k takes part iff k is in the neighbour set S; None is all nodes.
"""
import numpy as np

from tiled_model import set_cells

# WRONG rules, test aids that show the inputs tell them from the contract: "swapped" exchanges the two sets, "rows_only" ignores the
# neighbour set, "nbrs_only" ignores the row set, "lsb_first" reads both bitmaps with node i at bit i & 31
WRONG_RULES = ("swapped", "rows_only", "nbrs_only", "lsb_first")


def bitmap_words(n):
    return (n + 127) // 128 * 4


def bitmap(flags):
    """uint32 [S128(n) * 4] of the bool flags [n]: MSB first, the pad bits and pad words zero."""
    flags = np.asarray(flags, dtype=bool)
    bits = np.zeros(bitmap_words(flags.size) * 32, dtype=bool)
    bits[: flags.size] = flags
    w = bits.reshape(-1, 32).astype(np.uint64) << np.arange(31, -1, -1, dtype=np.uint64)
    return w.sum(axis=1).astype(np.uint32)


def members(words, n, lsb_first=False):
    """bool [n]: the nodes a bitmap names; ``lsb_first`` is the wrong reading (node i at bit i & 31)."""
    words = np.asarray(words).view(np.uint32)
    i = np.arange(n)
    shift = (i & 31) if lsb_first else 31 - (i & 31)
    return ((words[i >> 5] >> shift.astype(np.uint32)) & 1).astype(bool)


def _set(flags, n, wrong):
    if flags is None:
        return np.ones(n, dtype=bool)
    flags = np.asarray(flags, dtype=bool)
    assert flags.shape == (n,)
    return members(bitmap(flags), n, lsb_first=True) if wrong == "lsb_first" else flags


def induced_edges(src, dst, n, R, S, transposed=False, wrong=None):
    """(src, dst) int64: the set cells of the edge list's 1-bit adjacency (tiled_model.set_cells: multiplicities quantised) whose
    output-row end lies in R and whose neighbour end lies in S on this view (``transposed``: the output row is A's column), each once,
    sorted by (row, column). Cells of A, so the existing models take the list with the same ``transposed``."""
    assert wrong is None or wrong in WRONG_RULES
    if wrong == "swapped":
        R, S = S, R
    elif wrong == "rows_only":
        S = None
    elif wrong == "nbrs_only":
        R = None
    R, S = _set(R, n, wrong), _set(S, n, wrong)
    cells = set_cells(src, dst, n)
    r, c = cells // n, cells % n
    out, nbr = (c, r) if transposed else (r, c)
    k = R[out] & S[nbr]
    return r[k], c[k]
