"""tests/tiled_codes_model.py on its own (no GPU): the model's codes are ``am.quantise``, byte for byte; its buffer has the pad bytes of
the C entry; its sums are the exact neighbour sums; and its fused aggregate equals ``am.aggregate`` - the planes route's model - bit for
bit on every sweep input: Gaussian features at four ranges, the tie inputs of ``am.tie_inputs``, NaN and +-inf, on both views, with and
without masks and a row scale."""
import numpy as np
import pytest

import affine_model as am
import tiled_codes_model as cm
from tiled_model import random_edges

F32 = np.float32
BITS = (1, 2, 4, 8)
RANGES = ((1.0, 0.0), (10.0, 3.0), (0.1, -0.5), (100.0, 40.0))


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def sweep_inputs(n, N, bits, seed=0):
    """(name, float32 [n, N]) of every input the sweep runs."""
    rng = np.random.default_rng(seed)
    for k, (s, o) in enumerate(RANGES):
        yield f"gaussian x{s} + {o}", (rng.normal(size=(n, N)) * s + o).astype(F32)
    ties = am.tie_inputs(bits)[0]
    yield "ties", np.resize(ties, (n, N)).astype(F32)
    x = rng.normal(size=(n, N)).astype(F32)
    x[rng.integers(0, n, 7), rng.integers(0, N, 7)] = np.nan
    x[rng.integers(0, n, 7), rng.integers(0, N, 7)] = np.inf
    x[rng.integers(0, n, 7), rng.integers(0, N, 7)] = -np.inf
    yield "nan and inf", x
    yield "nothing finite", np.full((n, N), np.nan, F32)
    yield "zeros", np.zeros((n, N), F32)


@pytest.mark.parametrize("bits", BITS)
def test_the_codes_are_those_of_quantise(bits):
    for name, x in sweep_inputs(33, 7, bits):
        for per_column in (False, True):
            qp = am.qparams(x, bits, per_column)
            q = cm.codes(x, qp, bits)
            assert q.dtype == np.uint8 and (q.astype(np.int32) == am.quantise(x, qp, bits)).all(), name
            buf = cm.codes_buffer(x, qp, bits, ld=16, fill=0xA5)
            assert (buf[:, :7] == q).all() and (buf[:, 7:8] == 0).all() and (buf[:, 8:] == 0xA5).all(), name
    ties = am.tie_inputs(bits)
    assert (cm.codes(ties, am.qparams(ties, bits), bits) == am.quantise(ties, am.qparams(ties, bits), bits)).all()


def test_the_sums_are_the_neighbour_sums():
    n, N = 70, 5
    src, dst = random_edges(np.random.default_rng(1), n, 3 * n)
    rng = np.random.default_rng(2)
    Q = rng.integers(0, 256, size=(n, N)).astype(np.uint8)
    R, S = rng.random(n) < 0.5, rng.random(n) < 0.5
    for transposed in (False, True):
        A = am.dense_view(src, dst, n, transposed)
        got = cm.tiled_mm_codes(A, Q, R, S)
        assert got.dtype == np.int32
        for o in range(n):
            want = sum((Q[k].astype(np.int64) for k in range(n) if A[o, k] and R[o] and S[k]), np.zeros(N, np.int64))
            assert (got[o] == want).all()
        assert (cm.tiled_mm_codes(A, Q, np.ones(n, bool), None) == cm.tiled_mm_codes(A, Q)).all()


@pytest.mark.parametrize("transposed", [False, True], ids=["adj", "adjT"])
@pytest.mark.parametrize("bits", BITS)
def test_the_fused_aggregate_is_the_planes_aggregate(bits, transposed):
    n, N = 100, 6
    src, dst = random_edges(np.random.default_rng(3), n, 3 * n)
    A = am.dense_view(src, dst, n, transposed)
    rng = np.random.default_rng(4)
    R, S = rng.random(n) < 0.5, rng.random(n) < 0.5
    mean = am.inv_degree(am.masked_view(A, R, S).sum(axis=1))
    wild = mean.copy()
    wild[~R] = np.nan           # a non-finite scale on a masked-out row: 0 * NaN on both routes
    for name, T in sweep_inputs(n, N, bits):
        for scale, rm, sm in ((None, None, None), (am.inv_degree(A.sum(axis=1)), None, None), (None, R, S), (mean, R, S), (wild, R, S),
                              (None, R, None), (None, None, S)):
            got, want = cm.aggregate(A, T, bits, scale, rm, sm), am.aggregate(A, T, bits, scale, rm, sm)
            assert got.dtype == np.float32 and same_bits(got, want), (name, scale is not None, rm is not None, sm is not None)
