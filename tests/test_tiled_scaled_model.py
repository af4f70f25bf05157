"""The NumPy model of the scaled tiled products (tests/tiled_scaled_model.py) against the C oracle, without a GPU: the scaled sums of
the edge list, quantised and packed, equal the oracle's dense route (bitmm2int on the packed dense adjacency, times the scale,
val2bit) in both directions; the degrees equal the row and column sums of the quantised dense adjacency; a scale of ones gives the
unscaled words wherever the value quantiser of fl32(s) equals requant(s); and a mean never leaves 0 .. 2^b - 1."""
import numpy as np
import pytest

from oracle.qgtc_oracle import np_pack_edges, np_quantize, np_dense_adjacency
from tiled_model import aggregate, expected_bits, random_edges
from tiled_scaled_model import degrees, expected_bits_scaled, mean_scale, scaled


def _special_scale(n):
    vals = np.array([0.0, -0.0, 1.0, 0.5, -1.0, np.inf, -np.inf, np.nan, 2.0 ** 20, 2.0 ** -20], dtype=np.float32)
    return vals[np.arange(n) % vals.size]


@pytest.mark.parametrize("n,N,w,ob", [(1, 1, 1, 1), (33, 17, 2, 2), (161, 40, 8, 32), (400, 130, 3, 3), (129, 7, 5, 9)])
@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("kind", ["mean", "random", "special"])
def test_model_equals_the_oracle_on_the_dense_packing(oracle, n, N, w, ob, transposed, kind):
    rng = np.random.default_rng(n + N + w)
    src, dst = random_edges(rng, n, 5 * n + 3)
    Xq = rng.integers(0, 2 ** w, size=(n, N))
    deg = degrees(src, dst, n)[1 if transposed else 0]
    scale = {"mean": mean_scale(deg), "random": rng.uniform(2.0 ** -10, 4.0, n).astype(np.float32), "special": _special_scale(n)}[kind]
    y = scaled(aggregate(src, dst, n, Xq, transposed), scale)
    row, col = (dst, src) if transposed else (src, dst)
    oA = np_pack_edges(row, col, n, n, 1)
    oX = oracle.val2bit(Xq.astype(np.float32), w, True)
    with np.errstate(invalid="ignore", over="ignore"):
        dense = oracle.bitmm2int(oA, oX, n, n, N, 1, w, True) * scale[:, None]
    np.testing.assert_array_equal(y, dense)                      # NaN equals NaN here
    np.testing.assert_array_equal(expected_bits_scaled(oracle, y, ob), oracle.val2bit(dense, ob, False, False))


@pytest.mark.parametrize("n", [1, 33, 400])
def test_degrees_are_the_sums_of_the_quantised_dense_adjacency(n):
    src, dst = random_edges(np.random.default_rng(n), n, 5 * n + 3)
    A = np_quantize(np_dense_adjacency(src, dst, n, n), 1) & 1
    out_deg, in_deg = degrees(src, dst, n)
    np.testing.assert_array_equal(out_deg, A.sum(axis=1))
    np.testing.assert_array_equal(in_deg, A.sum(axis=0))
    s = mean_scale(out_deg)
    assert s.dtype == np.float32 and (s[out_deg == 0] == 0).all()
    assert (s[out_deg > 0] == (np.float64(1) / out_deg[out_deg > 0]).astype(np.float32)).all()   # one rounding


def _identity_sums():
    sums = list(range(600)) + list(range(2 ** 24 - 4, 2 ** 24 + 9)) + list(range(2 ** 25 - 4, 2 ** 25 + 9)) + [2 ** 31 - 129, 2 ** 31 - 1]
    for ob in range(1, 31):
        sums += [s for s in range(2 ** ob - 3, 2 ** ob + 4) if s >= 0]
    return np.unique(np.array(sums, dtype=np.int64))


def test_a_scale_of_ones_gives_the_unscaled_words(oracle):
    """quantise(fl32(s), ob) == requant(s, ob) for ob 1 .. 30 over small sums, 2^ob +- 3, the float32 integer edge (2^24, 2^25) and the
    largest sums: so row_scale = ones reproduces the unscaled output there. Checked value by value and as packed words."""
    sums = _identity_sums()
    ones = np.ones(sums.size, dtype=np.float32)
    y = scaled(sums[:, None], ones)
    for ob in range(1, 31):
        q = oracle.quantize(y, ob)[:, 0]
        want = np.array([oracle.requant(int(s), ob) for s in sums], dtype=np.int32)
        bad = np.flatnonzero(q != want)
        assert bad.size == 0, (ob, sums[bad][:5], q[bad][:5], want[bad][:5])
        np.testing.assert_array_equal(expected_bits_scaled(oracle, y, ob), expected_bits(oracle, sums[:, None], ob))


@pytest.mark.parametrize("b", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("transposed", [False, True])
def test_a_mean_stays_in_range(oracle, b, transposed):
    n, N = 700, 24
    rng = np.random.default_rng(b)
    src, dst = random_edges(rng, n, 9 * n)
    Xq = rng.integers(0, 2 ** b, size=(n, N))
    deg = degrees(src, dst, n)[1 if transposed else 0]
    y = scaled(aggregate(src, dst, n, Xq, transposed), mean_scale(deg))
    # fl32(s) * fl32(1 / d) with s <= d (2^b - 1) can exceed 2^b - 1 by a rounding error at most, far below the quantiser's 2^b compare
    assert (y <= np.float32(2 ** b - 1) * np.float32(1 + 2.0 ** -22)).all()
    q = oracle.quantize(y, b)
    assert q.min() >= 0 and q.max() <= 2 ** b - 1
    assert (q[deg == 0] == 0).all()
