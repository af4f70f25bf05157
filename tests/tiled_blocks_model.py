"""Exact NumPy model of mini-batch sampling on the tile-compressed adjacency (include/qgtc_blocks.h; qgtc_ppopp22_amd.fanout's
``sample_fanout(..., row_mask=, nbr_mask=)``, ``frontier`` and ``sample_blocks``), on top of tests/tiled_fanout_model.py: the thresholds
and counts of a fixed-fanout sample of an induced subgraph, its kept edges, its frontier as a bitmap and the chain of blocks. No GPU.

A node set is a bool [n] array here (``flags``); ``bitmap`` / ``flags_of`` convert to and from the int32 words of ``tiled.node_bitmap``
(node i at word i >> 5, bit 31 - (i & 31), S128(n) * 4 words, pad bits zero). On ``axis`` "row" the sampled node u of cell (i, j) is i
and its neighbour v is j; on "col" u = j and v = i. ``row`` restricts u, ``nbr`` restricts v; None means all nodes.

The thresholds are computed node by node from the definition - the k-th largest hash over the node's cells whose other end is in ``nbr``
- and NOT by re-packing: ``induced_edges`` is there so that a test can compare the two."""
import numpy as np

import tiled_fanout_model as fm
from tiled_drop_model import H

GOLDEN64 = 0x9E3779B97F4A7C15


def words_of(n):
    return (n + 127) // 128 * 4


def bitmap(flags):
    """int32 [S128(n) * 4] of a bool [n]"""
    flags = np.asarray(flags, dtype=bool)
    bits = np.zeros(words_of(len(flags)) * 32, dtype=bool)
    bits[:len(flags)] = flags
    return np.packbits(bits.reshape(-1, 32), axis=1, bitorder="big").view(">u4").astype(np.uint32).reshape(-1).view(np.int32)


def flags_of(words, n):
    """bool [n] of a bitmap, after asserting that its pad bits are zero and its length right"""
    words = np.ascontiguousarray(words).view(np.uint32)
    assert words.shape == (words_of(n),)
    bits = np.unpackbits(words.astype(">u4").view(np.uint8).reshape(-1, 4), axis=1, bitorder="big").reshape(-1).astype(bool)
    assert not bits[n:].any(), "pad bits must be zero"
    return bits[:n]


def _all(flags, n):
    return np.ones(n, dtype=bool) if flags is None else np.asarray(flags, dtype=bool)


def _ends(src, dst, n, axis):
    """(r, c, u, v): the set cells sorted by (row, column), the sampled end and the neighbour end of each"""
    assert axis in fm.AXES
    r, c = fm._cells(src, dst, n)
    return (r, c, r, c) if axis == "row" else (r, c, c, r)


def induced_edges(src, dst, n, axis, row=None, nbr=None):
    """(src, dst): the set cells with the sampled end in ``row`` and the neighbour end in ``nbr`` - what a user re-packs today"""
    r, c, u, v = _ends(src, dst, n, axis)
    keep = _all(row, n)[u] & _all(nbr, n)[v]
    return r[keep], c[keep]


def thresholds_counts(src, dst, n, k, seed, axis, row=None, nbr=None):
    """(thr uint32 [n], kept int32 [n]) of the masked sample, node by node from the definition"""
    assert k >= 1
    r, c, u, v = _ends(src, dst, n, axis)
    row, nbr = _all(row, n), _all(nbr, n)
    h = H(r, c, seed)
    thr, kept = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.int32)
    order = np.argsort(u, kind="stable")
    start = np.searchsorted(u[order], np.arange(n + 1))
    for node in np.nonzero(row)[0]:
        mine = order[start[node]:start[node + 1]]
        hs = np.sort(h[mine][nbr[v[mine]]])[::-1]
        kept[node] = min(len(hs), k)
        if len(hs) > k:
            thr[node] = hs[k - 1]
    return thr, kept


def degrees_masked(src, dst, n, axis, row=None, nbr=None):
    """int64 [n]: deg_m of the nodes of ``row``, 0 elsewhere"""
    ir, ic = induced_edges(src, dst, n, axis, row, nbr)
    return np.bincount(ir if axis == "row" else ic, minlength=n)


def kept_edges(src, dst, n, k, seed, axis, row=None, nbr=None):
    """(src, dst) int64: the cells the masked sample keeps, sorted by (row, column): an edge list of its own"""
    r, c, u, v = _ends(src, dst, n, axis)
    thr, _ = thresholds_counts(src, dst, n, k, seed, axis, row, nbr)
    keep = _all(row, n)[u] & _all(nbr, n)[v] & (H(r, c, seed) >= thr[u])
    return r[keep], c[keep]


def frontier(src, dst, n, k, seed, axis, row=None, nbr=None, include=None):
    """bool [n]: the neighbour ends of the kept cells, ORed with ``include``"""
    ks, kd = kept_edges(src, dst, n, k, seed, axis, row, nbr)
    out = np.zeros(n, dtype=bool)
    out[kd if axis == "row" else ks] = True
    return out if include is None else out | np.asarray(include, dtype=bool)


def layer_seed(seed, L, l):
    return (seed + (L - 1 - l) * GOLDEN64) % (1 << 64)


def blocks(src, dst, n, axis, seeds, fanouts, seed):
    """The chain of ``sample_blocks``, input layer first: dicts with rows (bool [n]), k, seed, thr, kept, inputs (bool [n])."""
    L, rows, out = len(fanouts), np.asarray(seeds, dtype=bool), []
    for l in range(L - 1, -1, -1):
        s = layer_seed(seed, L, l)
        thr, kept = thresholds_counts(src, dst, n, fanouts[l], s, axis, rows)
        inputs = frontier(src, dst, n, fanouts[l], s, axis, rows, None, rows)
        out.append(dict(rows=rows, k=fanouts[l], seed=s, thr=thr, kept=kept, inputs=inputs))
        rows = inputs
    return out[::-1]
