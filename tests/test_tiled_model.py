"""The NumPy model of the tiled adjacency (tests/tiled_model.py) against the C oracle, without a GPU: the exact sums of the edge list,
requantised and packed, equal oracle.bitmm2bit / bitmm2int on the dense packing of the same graph, forward and transposed; the tiles
model holds exactly the dense words."""
import numpy as np
import pytest

from qgtc_ppopp22_amd.shapes import P8, S128
from tiled_model import aggregate, expected_bits, expected_floats, np_colindex, np_tiled, random_edges, requant, variant


def _dense(src, dst, n):
    A = np.zeros((n, n), dtype=np.float32)
    np.add.at(A, (src, dst), 1.0)
    return A


@pytest.mark.parametrize("n,N,w,ob", [(1, 1, 1, 1), (33, 17, 2, 3), (161, 40, 8, 32), (400, 130, 3, 24), (129, 7, 5, 2)])
@pytest.mark.parametrize("transposed", [False, True])
def test_model_equals_the_oracle_on_the_dense_packing(oracle, n, N, w, ob, transposed):
    rng = np.random.default_rng(n + N + w)
    src, dst = random_edges(rng, n, 5 * n + 3)
    Xq = rng.integers(0, 2 ** w, size=(n, N))
    C = aggregate(src, dst, n, Xq, transposed)
    oA = oracle.val2bit(_dense(dst, src, n) if transposed else _dense(src, dst, n), 1)
    oX = oracle.val2bit(Xq.astype(np.float32), w, True)
    np.testing.assert_array_equal(expected_bits(oracle, C, ob), oracle.bitmm2bit(oA, oX, n, n, N, 1, w, ob))
    np.testing.assert_array_equal(expected_floats(C), oracle.bitmm2int(oA, oX, n, n, N, 1, w, True))


def test_model_sums_in_small_feature_chunks(oracle):
    """The chunked gather (a budget of a few values) gives the same sums as one gather."""
    n, N = 300, 37
    rng = np.random.default_rng(9)
    src, dst = random_edges(rng, n, 8 * n)
    Xq = rng.integers(0, 256, size=(n, N))
    for transposed in (False, True):
        np.testing.assert_array_equal(aggregate(src, dst, n, Xq, transposed, budget=5), aggregate(src, dst, n, Xq, transposed))


def test_model_quantises_multiplicities_per_cell():
    n = 10
    src = np.array([1] + [2] * 2 + [3] * 3 + [4] * 4 + [5, 5, 9], dtype=np.int64)
    dst = np.array([0] + [0] * 2 + [0] * 3 + [0] * 4 + [5, 5, 5], dtype=np.int64)   # (5, 5): a doubled self loop
    Xq = np.arange(1, n + 1)[:, None] * np.array([[1, 100]])
    fwd, tr = aggregate(src, dst, n, Xq), aggregate(src, dst, n, Xq, True)
    np.testing.assert_array_equal(fwd[:, 0], [0, 1, 0, 1, 1, 0, 0, 0, 0, 6])
    np.testing.assert_array_equal(tr[:, 1], [100 * (2 + 4 + 5), 0, 0, 0, 0, 100 * 10, 0, 0, 0, 0])


def test_tiles_model_holds_the_dense_words(oracle):
    n = 1000
    src, dst = random_edges(np.random.default_rng(2), n, 6 * n)
    row_ptr, kquad, tiles = np_tiled(src, dst, n)
    words = np.zeros(((n + 31) // 32 * 32, S128(n) * 4), dtype=np.uint32)
    rb = np.repeat(np.arange(row_ptr.size - 1), np.diff(row_ptr))
    for t in range(kquad.size):
        words[rb[t] * 32: rb[t] * 32 + 32, kquad[t] * 4: kquad[t] * 4 + 4] = tiles[t]
    dense = oracle.val2bit(_dense(src, dst, n), 1).reshape(P8(n), S128(n) * 4)
    np.testing.assert_array_equal(words[:n], dense[:n])
    assert not words[n:].any() and not dense[n:].any()
    # the generator's promises: an empty row block and an empty k-quad
    assert row_ptr[1] == row_ptr[2]
    col_ptr, _, _ = np_colindex(row_ptr, kquad, n)
    assert col_ptr[1] == col_ptr[2]


def test_requant_at_the_float_compare_edge(oracle):
    C = np.array([2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 25 + 1, 0, 7])
    assert requant(oracle, C, 24).tolist() == [2 ** 24 - 1, 2 ** 24, 2 ** 24, 2 ** 24 - 1, 0, 7]    # float(2^24 + 1) == 2^24
    assert requant(oracle, C, 23).tolist() == [2 ** 23 - 1] * 4 + [0, 7]
    assert requant(oracle, C, 32).tolist() == [2 ** 24 - 1, 2 ** 24, 2 ** 24, 2 ** 25, 0, 7]      # through float32 at any ob


def test_variant_map():
    assert [variant(N, False) for N in (1, 16, 17, 32, 33, 64, 65, 1000)] == [2, 2, 4, 4, 8, 8, 16, 16]
    assert [variant(N, True) for N in (1, 16, 17, 32, 33, 64, 65, 1000)] == [8, 8, 16, 16, 32, 32, 64, 64]
