"""The float tiled products' model (tests/tiled_float_model.py) against three independent statements: on integers it is the exact
edge-list aggregate of tests/tiled_model.py; on floats it stays within the standard error bound of a recursive float32 sum around the
float64 sum; and on the inputs the device sweep uses the ORDER of the adds is visible in the result, so a kernel that adds in another
order cannot equal the model by luck. No GPU."""
import numpy as np
import pytest

from tiled_float_model import (FLOAT_FORWARD_VARIANTS, FLOAT_TRANSPOSED_VARIANTS, aggregate_f32, float_chunks, float_variant,
                               neighbour_lists)
from tiled_model import aggregate, random_edges
from tiled_scaled_model import degrees, mean_scale, scaled

SIZES = [1, 31, 97, 1000, 4097]


def _graph(n):
    rng = np.random.default_rng(500 + n)
    return rng, random_edges(rng, n, 6 * n + 5)


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_integers_equal_the_exact_aggregate(n, transposed):
    """Integer X with every partial sum below 2^24: all float32 adds are exact, so the model is the int64 aggregate, also scaled."""
    rng, (src, dst) = _graph(n)
    Xq = rng.integers(0, 256, size=(n, 7))
    C = aggregate(src, dst, n, Xq, transposed)
    assert C.max() < 2 ** 24
    got = aggregate_f32(src, dst, n, Xq.astype(np.float32), transposed)
    np.testing.assert_array_equal(got.view(np.uint32), C.astype(np.float32).view(np.uint32))
    deg = degrees(src, dst, n)[1 if transposed else 0]
    np.testing.assert_array_equal(neighbour_lists(src, dst, n, transposed)[2], deg)
    s = mean_scale(deg)
    np.testing.assert_array_equal(aggregate_f32(src, dst, n, Xq.astype(np.float32), transposed, s).view(np.uint32),
                                  scaled(C, s).view(np.uint32))


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_floats_stay_within_the_recursive_sum_bound(n, transposed):
    """|model - float64 sum| <= (d - 1) * 2^-24 * sum_k |X[v_k, c]| * (1 + small), d the row's degree (Higham, recursive summation:
    gamma_{d-1} = (d-1)u / (1 - (d-1)u) with u = 2^-24; d <= 4097 here, so the factor 1 + small = 1.001 covers the denominator)."""
    rng, (src, dst) = _graph(n)
    N = 20
    X = rng.standard_normal((n, N)).astype(np.float32)
    got = aggregate_f32(src, dst, n, X, transposed).astype(np.float64)
    out_row, nb, deg = neighbour_lists(src, dst, n, transposed)
    exact, mag = np.zeros((n, N)), np.zeros((n, N))
    np.add.at(exact, out_row, X[nb].astype(np.float64))
    np.add.at(mag, out_row, np.abs(X[nb]).astype(np.float64))
    bound = np.maximum(deg - 1, 0)[:, None] * 2.0 ** -24 * mag * 1.001
    assert (np.abs(got - exact) <= bound).all()
    assert (got[deg == 0] == 0).all() and not np.signbit(got[deg == 0]).any()      # a row without neighbours: +0
    one = deg == 1
    if one.any():                                                                    # one neighbour: its row, untouched
        first = np.concatenate([[0], np.cumsum(deg)[:-1]])
        np.testing.assert_array_equal(got[one].astype(np.float32), X[nb[first[one]]])


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("N", [20, 64])
@pytest.mark.parametrize("n", [31, 97, 1000, 4097])
def test_the_order_matters_on_the_sweeps_inputs(n, N, transposed):
    """Standard-normal X and N >= 16: at least 90 % of the rows of degree >= 3 differ somewhere from the same sum in descending
    neighbour order. A condition on the inputs of the device sweep, not a measurement of any kernel."""
    rng, (src, dst) = _graph(n)
    X = rng.standard_normal((n, N)).astype(np.float32)
    up = aggregate_f32(src, dst, n, X, transposed)
    down = aggregate_f32(src, dst, n, X, transposed, descending=True)
    deg = neighbour_lists(src, dst, n, transposed)[2]
    rows = deg >= 3
    assert rows.sum() >= 5
    differ = (up.view(np.uint32) != down.view(np.uint32)).any(axis=1)
    assert differ[rows].mean() >= 0.9, differ[rows].mean()
    assert not differ[deg <= 2].any()              # one add, or two that commute


def test_nan_and_inf_reach_exactly_the_adjacent_rows():
    n, N = 300, 5
    rng, (src, dst) = _graph(n)
    X = rng.standard_normal((n, N)).astype(np.float32)
    X[7, 0], X[n // 3, 1], X[200, 2] = np.nan, np.inf, -np.inf
    for transposed in (False, True):
        out_row, nb, _ = neighbour_lists(src, dst, n, transposed)
        got = aggregate_f32(src, dst, n, X, transposed)
        for v, c in ((7, 0), (n // 3, 1), (200, 2)):
            touched = np.zeros(n, bool)
            touched[out_row[nb == v]] = True
            np.testing.assert_array_equal(~np.isfinite(got[:, c]), touched)
        assert np.isfinite(got[:, 3:]).all()


def test_the_variant_table():
    assert [float_variant(N, False) for N in (1, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257)] == \
        [(16, 1), (16, 1), (16, 2), (16, 2), (16, 4), (16, 4), (32, 4), (32, 4), (64, 4), (64, 4), (64, 4)]
    assert [float_variant(N, True) for N in (1, 16, 17, 32, 33, 64, 65)] == [(16, 1), (16, 1), (16, 2), (16, 2), (16, 4), (16, 4), (16, 4)]
    assert [float_chunks(N, False) for N in (1, 128, 129, 256, 257, 383)] == [1, 1, 1, 1, 2, 2]
    assert [float_chunks(N, True) for N in (1, 64, 65, 128, 129, 383)] == [1, 1, 2, 2, 3, 6]
    assert len(FLOAT_FORWARD_VARIANTS) == 5 and len(FLOAT_TRANSPOSED_VARIANTS) == 3
