"""The model of the extremum tiled products (tests/tiled_max_model.py) against a brute-force dense loop and against torch's CPU autograd:
ties, signed zeros, NaN, infinities and empty rows, inputs that tell the tie rule and the NaN rule from their opposites, and the select as
the vector-Jacobian product. No GPU."""
import numpy as np
import pytest

from tiled_max_model import MAX, MIN, extremum_f32, select_f32
from tiled_model import random_edges, set_cells


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_floats(got, want):
    """assert_floats_identical's rule: bit for bit, any NaN equals any NaN."""
    gn, wn = np.isnan(got), np.isnan(want)
    return got.shape == want.shape and np.array_equal(gn, wn) and np.array_equal(bits(got)[~gn], bits(want)[~wn])


def dense_mask(src, dst, n, transposed):
    cells = set_cells(src, dst, n)
    A = np.zeros((n, n), bool)
    A[cells // n, cells % n] = True
    return A.T.copy() if transposed else A


def brute_extremum(A, X, op):
    """The fold of include/qgtc.h, element by element in Python."""
    n, N = X.shape
    out, arg = np.zeros((n, N), np.float32), np.full((n, N), -1, np.int32)
    for r in range(n):
        nb = np.flatnonzero(A[r])
        for c in range(N):
            if nb.size == 0:
                continue
            a, s = nb[0], X[nb[0], c]
            for v in nb[1:]:
                x = X[v, c]
                if not np.isnan(s) and (np.isnan(x) or (x < s if op == MIN else x > s)):
                    s, a = x, v
            out[r, c], arg[r, c] = s, a
    return out, arg


def brute_select(A, dY, arg):
    n, N = dY.shape
    out = np.zeros((n, N), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for v in range(n):
            for c in range(N):
                s = np.float32(0.0)
                for r in np.flatnonzero(A[v]):
                    if arg[r, c] == v:
                        s = np.float32(s + dY[r, c])
                out[v, c] = s
    return out


def special_values(rng, n, N):
    """Few distinct values, so nearly every element is a tie, with both zeros, both infinities and NaNs among them."""
    pool = np.array([-2.0, -1.0, -0.0, 0.0, 1.0, 1.0, 3.0, np.inf, -np.inf, np.nan], np.float32)
    return pool[rng.integers(0, pool.size, size=(n, N))]


@pytest.mark.parametrize("n", [1, 2, 9, 33, 70])
def test_the_model_is_the_dense_fold(n):
    rng = np.random.default_rng(n)
    src, dst = random_edges(rng, n, 3 * n + 2)
    if n >= 9:                                     # rows and columns without any neighbour
        keep = (src != 4) & (dst != 4) & (src != 7) & (dst != 6)
        src, dst = src[keep], dst[keep]
    for X in (rng.standard_normal((n, 5)).astype(np.float32), special_values(rng, n, 6)):
        for transposed in (False, True):
            A = dense_mask(src, dst, n, transposed)
            if n >= 9:
                assert not A[4].any()
            for op in (MAX, MIN):
                out, arg = extremum_f32(src, dst, n, X, transposed, op)
                want, warg = brute_extremum(A, X, op)
                assert same_floats(out, want), (n, transposed, op)
                np.testing.assert_array_equal(arg, warg)
                assert out.dtype == np.float32 and arg.dtype == np.int32
                # the value is the winner's own word; a row without neighbours gives (+0, -1)
                has = arg >= 0
                cols = np.broadcast_to(np.arange(X.shape[1]), arg.shape)
                assert same_floats(out[has], X[arg[has], cols[has]])
                np.testing.assert_array_equal(has, np.broadcast_to(A.any(axis=1)[:, None], arg.shape))
                assert (bits(out)[~has] == 0).all()
                dY = special_values(rng, n, X.shape[1])
                assert same_floats(select_f32(src, dst, n, dY, arg, not transposed), brute_select(A.T, dY, arg))
                junk = rng.integers(-3, n + 3, size=arg.shape).astype(np.int32)
                assert same_floats(select_f32(src, dst, n, dY, junk, transposed), brute_select(A, dY, junk))


def test_worked_cases():
    """Row 0 sees 1, 2, 3; row 1 sees 0; row 2 sees nobody."""
    src, dst, n = np.array([0, 0, 0, 1]), np.array([1, 2, 3, 0]), 4
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    #             ties   -0/+0  +0/-0  NaN first  NaN later  two NaNs  infinities
    X = np.array([[9.0,  9.0,   9.0,   9.0,       9.0,       9.0,      9.0],
                  [5.0,  -0.0,  0.0,   nan,       1.0,       nan,      -inf],
                  [5.0,  0.0,   -0.0,  7.0,       nan,       nan,      inf],
                  [5.0,  -1.0,  -1.0,  8.0,       99.0,      3.0,      inf]], np.float32)
    out, arg = extremum_f32(src, dst, n, X, False, MAX)
    np.testing.assert_array_equal(arg[0], [1, 1, 1, 1, 2, 1, 2])
    np.testing.assert_array_equal(bits(out[0])[[0, 1, 2, 6]], bits(np.array([5.0, -0.0, 0.0, inf], np.float32)))
    assert np.isnan(out[0, 3:6]).all()
    np.testing.assert_array_equal(arg[1], [0] * 7)
    np.testing.assert_array_equal(arg[2:], -1)
    assert (bits(out[2:]) == 0).all()
    out, arg = extremum_f32(src, dst, n, X, False, MIN)
    np.testing.assert_array_equal(arg[0], [1, 3, 3, 1, 2, 1, 1])
    assert out[0, 6] == -inf
    # transposed: column 0 is seen from row 1 only, columns 1 .. 3 from row 0
    out, arg = extremum_f32(src, dst, n, X, True, MAX)
    np.testing.assert_array_equal(arg[:, 0], [1, 0, 0, 0])
    # the select gives a tie's whole gradient to the winner
    _, arg = extremum_f32(src, dst, n, X, False, MAX)
    dY = np.arange(1, 29, dtype=np.float32).reshape(4, 7)
    g = select_f32(src, dst, n, dY, arg, True)
    np.testing.assert_array_equal(g[:, 0], [8.0, 1.0, 0.0, 0.0])       # X[0] wins row 1, X[1] wins row 0's three-way tie
    assert g.sum() == dY[:2].sum()                                      # rows 2 and 3 have no neighbour: their dY goes nowhere


@pytest.mark.parametrize("n", [33, 70])
def test_the_inputs_tell_the_rules_apart(n):
    """On the tie inputs a model with the opposite tie rule (highest id) and one that ignores NaN differ from the model."""
    rng = np.random.default_rng(100 + n)
    src, dst = random_edges(rng, n, 4 * n)
    ties = rng.integers(0, 3, size=(n, 4)).astype(np.float32)
    nans = np.where(rng.random((n, 4)) < 0.2, np.float32(np.nan), rng.standard_normal((n, 4)).astype(np.float32))
    for transposed in (False, True):
        for op in (MAX, MIN):
            out, arg = extremum_f32(src, dst, n, ties, transposed, op)
            out_h, arg_h = extremum_f32(src, dst, n, ties, transposed, op, highest_id=True)
            assert same_floats(out, out_h) and (arg != arg_h).any() and (arg <= arg_h).all()
            out, arg = extremum_f32(src, dst, n, nans, transposed, op)
            out_i, arg_i = extremum_f32(src, dst, n, nans, transposed, op, ignore_nan=True)
            assert not same_floats(out, out_i) and (arg != arg_i).any()
            assert np.isnan(out).any() and not np.isnan(out_i[arg_i >= 0]).all()
    # signed zeros: the lower id keeps its sign, the opposite rule takes the other one
    src, dst = np.array([0, 0]), np.array([1, 2])
    Z = np.array([[1.0], [-0.0], [0.0]], np.float32)
    assert bits(extremum_f32(src, dst, 3, Z, False, MAX)[0])[0, 0] == 0x80000000
    assert bits(extremum_f32(src, dst, 3, Z, False, MAX, highest_id=True)[0])[0, 0] == 0


@pytest.mark.parametrize("n", [40, 70])
def test_the_select_is_the_vector_jacobian_product(n):
    """Tie-free X and integer-valued dY (sums exact in any order): the select on the other view equals torch's CPU autograd through a dense
    masked amax / amin."""
    import torch

    rng = np.random.default_rng(7 * n)
    src, dst = random_edges(rng, n, 4 * n)
    N = 6
    X = rng.permutation(n * N).reshape(n, N).astype(np.float32) - n * N // 2       # all values distinct
    dY = rng.integers(-8, 9, size=(n, N)).astype(np.float32)
    for transposed in (False, True):
        A = torch.from_numpy(dense_mask(src, dst, n, transposed))
        for op in (MAX, MIN):
            Xt = torch.from_numpy(X).requires_grad_(True)
            fill = float("inf") if op == MIN else float("-inf")
            masked = torch.where(A[:, :, None], Xt[None, :, :], torch.tensor(fill))
            ref = masked.amin(dim=1) if op == MIN else masked.amax(dim=1)
            ref = torch.where(A.any(dim=1)[:, None], ref, torch.zeros(()))
            (grad,) = torch.autograd.grad(ref, Xt, torch.from_numpy(dY))
            out, arg = extremum_f32(src, dst, n, X, transposed, op)
            np.testing.assert_array_equal(bits(out), bits(ref.detach().numpy()))
            got = select_f32(src, dst, n, dY, arg, not transposed)
            np.testing.assert_array_equal(bits(got), bits(grad.numpy()))
            wins = (arg.astype(np.int64) * N + np.arange(N))[arg >= 0]
            assert np.bincount(wins).max() >= 2    # some element won more than one row: the select really adds
