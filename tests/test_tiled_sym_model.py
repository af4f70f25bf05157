"""The source-scale model (tests/tiled_sym_model.py) against independent statements: it is the float model on the pre-multiplied
matrix bit for bit; it stays within the derived bound of the float64 result; on the inputs the device sweep uses a fused multiply-add
is visible in the result, so a contracted kernel cannot equal the model by luck; the inverse square roots at the degrees that matter;
and QGTC.add_self_loops on lists that already hold loops. No GPU."""
import numpy as np
import pytest

from tiled_float_model import aggregate_f32, neighbour_lists
from tiled_model import random_edges, set_cells
from tiled_sym_model import add_self_loops, aggregate_f32_src, error_bound, inv_sqrt_degree

SIZES = [1, 31, 97, 1000, 4097]


def _graph(n):
    rng = np.random.default_rng(1500 + n)
    return rng, random_edges(rng, n, 6 * n + 5)


def _scales(rng, src, dst, n, transposed):
    """(row scale, source scale) of the symmetric normalisation on this view, and a random pair"""
    out_deg, in_deg = neighbour_lists(src, dst, n, False)[2], neighbour_lists(src, dst, n, True)[2]
    r, c = (in_deg, out_deg) if transposed else (out_deg, in_deg)
    return {"sym": (inv_sqrt_degree(r), inv_sqrt_degree(c)),
            "random": (rng.uniform(2.0 ** -10, 4.0, n).astype(np.float32), rng.uniform(-4.0, 4.0, n).astype(np.float32))}


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_equals_the_float_model_on_the_premultiplied_matrix(n, transposed):
    rng, (src, dst) = _graph(n)
    X = rng.standard_normal((n, 20)).astype(np.float32)
    for kind, (r, c) in _scales(rng, src, dst, n, transposed).items():
        pre = c[:, None] * X
        assert pre.dtype == np.float32
        for scale in (None, r):
            got = aggregate_f32_src(src, dst, n, X, transposed, scale, c)
            np.testing.assert_array_equal(got.view(np.uint32), aggregate_f32(src, dst, n, pre, transposed, scale).view(np.uint32), kind)
    np.testing.assert_array_equal(aggregate_f32_src(src, dst, n, X, transposed).view(np.uint32),
                                  aggregate_f32(src, dst, n, X, transposed).view(np.uint32))       # no source scale: the float model
    ones = np.ones(n, np.float32)
    np.testing.assert_array_equal(aggregate_f32_src(src, dst, n, X, transposed, None, ones).view(np.uint32),
                                  aggregate_f32(src, dst, n, X, transposed).view(np.uint32))       # a scale of ones: the same bits


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_stays_within_the_bound_of_the_float64_result(n, transposed):
    """|model - r sum c_v x_v| <= (d + 2) 2^-24 |r| sum |c_v x_v|: d + 1 roundings on a term's path through a row of degree d, plus
    the final multiply."""
    rng, (src, dst) = _graph(n)
    X = rng.standard_normal((n, 20)).astype(np.float32)
    for kind, (r, c) in _scales(rng, src, dst, n, transposed).items():
        for scale in (None, r):
            got = aggregate_f32_src(src, dst, n, X, transposed, scale, c).astype(np.float64)
            exact, bound = error_bound(src, dst, n, X, transposed, scale, c)
            err = np.abs(got - exact)
            assert (err <= bound).all(), (kind, float((err / np.maximum(bound, 1e-300)).max()))


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("N", [20, 64])
@pytest.mark.parametrize("n", [31, 97, 1000, 4097])
def test_a_fused_multiply_add_shows_on_the_sweeps_inputs(n, N, transposed):
    """Standard-normal X, N >= 16, the symmetric and a random scale: at least 90 % of the rows of degree >= 2 differ somewhere when
    every multiply and add is one fma. A condition on the inputs of the device sweep, not a measurement of any kernel."""
    rng, (src, dst) = _graph(n)
    X = rng.standard_normal((n, N)).astype(np.float32)
    deg = neighbour_lists(src, dst, n, transposed)[2]
    rows = deg >= 2
    assert rows.sum() >= 5
    for kind, (r, c) in _scales(rng, src, dst, n, transposed).items():
        two = aggregate_f32_src(src, dst, n, X, transposed, None, c)
        one = aggregate_f32_src(src, dst, n, X, transposed, None, c, fused=True)
        differ = (two.view(np.uint32) != one.view(np.uint32)).any(axis=1)
        assert differ[rows].mean() >= 0.9, (kind, differ[rows].mean())
        assert not differ[deg == 0].any()


def test_the_wrong_index_shows_on_the_sweeps_inputs():
    """The factor of the output row in place of the neighbour's changes nearly every row with a neighbour."""
    n, N = 1000, 20
    rng, (src, dst) = _graph(n)
    X = rng.standard_normal((n, N)).astype(np.float32)
    for transposed in (False, True):
        deg = neighbour_lists(src, dst, n, transposed)[2]
        _, c = _scales(rng, src, dst, n, transposed)["sym"]
        good = aggregate_f32_src(src, dst, n, X, transposed, None, c)
        bad = aggregate_f32_src(src, dst, n, X, transposed, None, c, by_output_row=True)
        assert (good.view(np.uint32) != bad.view(np.uint32)).any(axis=1)[deg >= 1].mean() >= 0.9


def test_inverse_square_roots():
    got = inv_sqrt_degree(np.array([0, 1, 2, 3, 4, 1 << 23], dtype=np.int32))
    assert got.dtype == np.float32
    want = np.array([0x00000000,      # degree 0: +0
                     0x3F800000,      # 1
                     0x3F3504F3,      # 1 / sqrt(2) = 0.70710678...: fl32(sqrt 2) = 0x3FB504F3, its reciprocal rounds to 0x3F3504F3
                     0x3F13CD3A,      # 1 / sqrt(3) = 0.57735027...
                     0x3F000000,      # 0.5
                     0x39B504F3],     # 2^-11.5 = 2^-12 sqrt(2)
                    dtype=np.uint32)
    np.testing.assert_array_equal(got.view(np.uint32), want)
    # against float64: the two float32 roundings stay within 1.5 ulp of the true value, and perfect squares are exact
    d = np.arange(1, 70000, dtype=np.int64)
    y = inv_sqrt_degree(d).astype(np.float64)
    assert (np.abs(y * np.sqrt(d.astype(np.float64)) - 1) <= 1.5 * 2.0 ** -24 * 2).all()
    sq = np.arange(1, 257, dtype=np.int64) ** 2
    pow4 = sq[(sq & (sq - 1)) == 0]
    np.testing.assert_array_equal(inv_sqrt_degree(pow4), (1.0 / np.sqrt(pow4)).astype(np.float32))


@pytest.mark.parametrize("copies", [0, 1, 2, 3])
def test_add_self_loops_keeps_exactly_one_loop_per_node(copies):
    """A list with no, one, two and three copies of the loops of some nodes: afterwards every node has exactly one, the other edges are
    untouched, and the packed adjacency (multiplicity 2 quantises to 0) has the whole diagonal set. Appending loops blindly would erase
    the diagonal where one copy was there and keep it where two were."""
    import torch

    from qgtc_ppopp22_amd.tiled import add_self_loops as torch_add_self_loops

    n = 50
    rng = np.random.default_rng(copies)
    src, dst = rng.integers(0, n, 300), rng.integers(0, n, 300)
    keep = src != dst
    src, dst = src[keep], dst[keep]
    looped = np.arange(0, n, 3)
    src = np.concatenate([src] + [looped] * copies)
    dst = np.concatenate([dst] + [looped] * copies)
    order = rng.permutation(src.size)
    src, dst = src[order], dst[order]
    s2, d2 = torch_add_self_loops(torch.from_numpy(src), torch.from_numpy(dst), n)
    assert s2.dtype == torch.int64 and d2.dtype == torch.int64
    s2, d2 = s2.numpy(), d2.numpy()
    ms, md = add_self_loops(src, dst, n)
    np.testing.assert_array_equal(s2, ms)
    np.testing.assert_array_equal(d2, md)
    loops = s2[s2 == d2]
    np.testing.assert_array_equal(np.sort(loops), np.arange(n))                    # exactly one per node
    off = src != dst
    np.testing.assert_array_equal(s2[: off.sum()], src[off])                       # the other edges, in their order
    np.testing.assert_array_equal(d2[: off.sum()], dst[off])
    cells = set_cells(s2, d2, n)
    assert np.isin(np.arange(n) * (n + 1), cells).all()                            # the diagonal survives the packer's quantiser
    if copies == 1:
        blind = set_cells(np.concatenate([src, np.arange(n)]), np.concatenate([dst, np.arange(n)]), n)
        assert not np.isin(looped * (n + 1), blind).any()                          # what blind appending would have done
