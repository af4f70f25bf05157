"""The NumPy model of the edge values (tests/tiled_edge_model.py) against a dense float64 product on integer-valued data, where every
sum is exact, and against itself across the views: the model on adj.T must equal the model on the reversed edge list with the values
permuted by the slots. No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import tiled_edge_model as em  # noqa: E402
from tiled_model import random_edges, set_cells  # noqa: E402


def graph(n, seed=0):
    rng = np.random.default_rng(seed)
    src, dst = random_edges(rng, n, max(4, n * 4))
    return np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)


def dense(src, dst, n, values):
    r, c = em.slot_cells(src, dst, n)
    W = np.zeros((n, n), dtype=np.float64)
    W[r, c] = values
    return W


@pytest.mark.parametrize("n", [1, 33, 129, 300])
def test_slot_order_and_index(n):
    src, dst = graph(n)
    r, c = em.slot_cells(src, dst, n)
    cells = set_cells(src, dst, n)
    assert r.size == cells.size and np.array_equal(np.sort(r * n + c), cells)
    tile_key = (r >> 5) * ((n + 127) // 128) + (c >> 7)
    # tile id, then tile row, then column, strictly ascending
    key = (tile_key * 32 + (r & 31)) * 128 + (c & 127)
    assert (np.diff(key) > 0).all()
    val_ptr, val_row = em.value_index(src, dst, n)
    assert val_ptr[-1] == r.size and val_row.dtype == np.int16 and val_row.max(initial=0) <= 31 * 128
    # slot(t, r, c) = val_ptr[t] + val_row[t][r] + the row's bits before c, for every stored cell
    _, tile_of = np.unique(tile_key, return_inverse=True)
    for s in range(r.size):
        before = np.count_nonzero((tile_key[:s] == tile_key[s]) & (r[:s] == r[s]))
        assert s == val_ptr[tile_of[s]] + val_row[tile_of[s], r[s] & 31] + before
    assert np.array_equal(em.edge_slots(src, dst, n, r, c), np.arange(r.size))
    assert em.edge_slots(src, dst, n, [-1, n, 0], [0, 0, n]).tolist() == [-1, -1, -1]


@pytest.mark.parametrize("n", [1, 33, 129, 300])
@pytest.mark.parametrize("transposed", [False, True])
def test_weighted_fold_is_the_dense_product_on_integers(n, transposed):
    src, dst = graph(n, 1)
    rng = np.random.default_rng(n)
    nnz = em.slot_cells(src, dst, n)[0].size
    values = rng.integers(-4, 5, nnz).astype(np.float32)
    X = rng.integers(-8, 9, (n, 5)).astype(np.float32)
    scale = rng.integers(1, 4, n).astype(np.float32)
    W = dense(src, dst, n, values)
    want = (W.T if transposed else W) @ X.astype(np.float64)
    assert np.abs(want).max(initial=0) * 3 < 2 ** 24
    assert np.array_equal(em.weighted_f32(src, dst, n, X, values, transposed).astype(np.float64), want)
    assert np.array_equal(em.weighted_f32(src, dst, n, X, values, transposed, scale).astype(np.float64), want * scale[:, None])


@pytest.mark.parametrize("n", [33, 300])
def test_transposed_view_is_the_reversed_graph_with_permuted_values(n):
    src, dst = graph(n, 2)
    rng = np.random.default_rng(7)
    r, c = em.slot_cells(src, dst, n)
    values = rng.normal(size=r.size).astype(np.float32)
    X = rng.normal(size=(n, 19)).astype(np.float32)
    # the reversed graph stores cell (c, r) for every (r, c); its slot order differs, the values follow their cells
    rr, rc = em.slot_cells(dst, src, n)
    perm = em.edge_slots(src, dst, n, rc, rr)
    assert (perm >= 0).all() and np.array_equal(np.sort(perm), np.arange(r.size))
    a = em.weighted_f32(src, dst, n, X, values, transposed=True)
    b = em.weighted_f32(dst, src, n, X, values[perm], transposed=False)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    A, B = rng.normal(size=(n, 70)).astype(np.float32), rng.normal(size=(n, 70)).astype(np.float32)
    sa = em.sddmm_f32(src, dst, n, A, B, transposed=True)
    sb = em.sddmm_f32(dst, src, n, A, B, transposed=False)
    assert np.array_equal(sa[perm].view(np.uint32), sb.view(np.uint32))


@pytest.mark.parametrize("N", [1, 64, 65, 300])
def test_sddmm_is_the_dense_product_on_integers(N):
    n = 129
    src, dst = graph(n, 3)
    rng = np.random.default_rng(N)
    A, B = rng.integers(-8, 9, (n, N)).astype(np.float32), rng.integers(-8, 9, (n, N)).astype(np.float32)
    r, c = em.slot_cells(src, dst, n)
    full = A.astype(np.float64) @ B.astype(np.float64).T
    assert np.array_equal(em.sddmm_f32(src, dst, n, A, B).astype(np.float64), full[r, c])
    assert np.array_equal(em.sddmm_f32(src, dst, n, A, B, transposed=True).astype(np.float64), full[c, r])


def test_variant_tables_restate_the_launcher():
    assert [em.edge_variant(N, False) for N in (1, 16, 17, 33, 64, 65, 129, 257, 300)] == [
        (16, 1), (16, 1), (16, 2), (16, 4), (16, 4), (32, 4), (64, 4), (64, 4), (64, 4)]
    assert [em.edge_variant(N, True) for N in (1, 16, 17, 33, 64, 65, 300)] == [(16, 1), (16, 1), (16, 2), (16, 4), (16, 4), (16, 4), (16, 4)]
    assert set(em.EDGE_FORWARD_VARIANTS) == {em.edge_variant(N, False) for N in (1, 17, 33, 65, 129)}
    assert set(em.EDGE_TRANSPOSED_VARIANTS) == {em.edge_variant(N, True) for N in (1, 17, 33)}
    assert [em.sddmm_variant(N) for N in (1, 256, 257)] == ["registers", "registers", "reread"]
