"""Exact NumPy model of edge dropout on the tile-compressed adjacency (include/qgtc.h, "Edge dropout"; ``edge_drop=`` of
QGTC.tiledMMFloat / QGTC.tiledAggregate): the 32-bit hash of a cell, the keep test and a filter over the set cells of
tests/tiled_model.py. Masking is dropping, so the filtered edge list feeds the float, extremum and attention models unchanged
(tests/tiled_float_model.py, tiled_sym_model.py, tiled_max_model.py, tiled_attn_model.py). No GPU.

A cell is row i, column j of A in the adjacency's own numbering, on either view. All arithmetic is uint32 and wraps:
    mix32(x):  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16
    k0 = seed & 0xffffffff,  k1 = seed >> 32,  K = mix32(k0) + k1
    R(i) = mix32(i ^ k0),  C(j) = mix32(j ^ k1) + 0x9E3779B9,  H = mix32((R(i) ^ C(j)) + K),  kept <=> H >= T = floor(rate * 2^32)
"""
import math

import numpy as np

from tiled_model import set_cells

U32 = np.uint32
GOLDEN = U32(0x9E3779B9)
SEEDS = (0, 1, 0x0123456789ABCDEF, 2 ** 64 - 1)

# WRONG rules, test aids that show the inputs tell them from the contract: ">" keeps H > T only, "transposed" hashes (j, i),
# "swapped_seed" exchanges the two seed words, "no_K" leaves K out of the combine
WRONG_RULES = (">", "transposed", "swapped_seed", "no_K")


def mix32(x):
    x = np.asarray(x, dtype=U32).copy()
    with np.errstate(over="ignore"):
        x ^= x >> U32(16)
        x *= U32(0x7FEB352D)
        x ^= x >> U32(15)
        x *= U32(0x846CA68B)
        x ^= x >> U32(16)
    return x


def threshold(rate):
    """T = floor(rate * 2^32), computed in double, for 0 <= rate < 1."""
    rate = float(rate)
    assert 0.0 <= rate < 1.0
    return int(math.floor(rate * 4294967296.0))


def H(i, j, seed, wrong=None):
    """uint32 hash of the cells (i, j) (arrays or scalars) under the 64-bit seed."""
    assert 0 <= seed < 2 ** 64 and (wrong is None or wrong in WRONG_RULES)
    i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
    if wrong == "transposed":
        i, j = j, i
    k0, k1 = U32(seed & 0xFFFFFFFF), U32(seed >> 32)
    if wrong == "swapped_seed":
        k0, k1 = k1, k0
    with np.errstate(over="ignore"):
        K = U32(0) if wrong == "no_K" else mix32(k0) + k1
        R = mix32(i.astype(U32) ^ k0)
        C = mix32(j.astype(U32) ^ k1) + GOLDEN
        return mix32((R ^ C) + K)


def kept(i, j, seed, T, wrong=None):
    """bool: the cells the mask keeps at threshold T (an int in [0, 2^32))."""
    assert 0 <= T < 2 ** 32
    h = H(i, j, seed, wrong)
    return (h > U32(T)) if wrong == ">" else (h >= U32(T))


def kept_edges(src, dst, n, T, seed, wrong=None):
    """(src, dst) int64: the set cells of the edge list's 1-bit adjacency (tiled_model.set_cells: multiplicities quantised) that the mask
    keeps, each once, sorted by (row, column). An edge list of its own: packing it gives the adjacency the masked operators must equal,
    and the existing models take it as it is."""
    cells = set_cells(src, dst, n)
    r, c = cells // n, cells % n
    k = kept(r, c, seed, T, wrong)
    return r[k], c[k]
