"""tests/affine_model.py on its own (no GPU): the range rules on special inputs, ties, the zero point, the half-step bound, the integer
identity of the dequantising epilogue, the two first-order error bounds against float64, per-column against per-tensor weights, and the
two-layer composition's error falling with the bit width. The seeds are fixed; where a property is not a theorem (per column no worse than
per tensor, the ordering of the composition's errors) the seed was chosen so that it holds, and the docstring says so."""
import numpy as np
import pytest

import affine_model as am
from tiled_model import random_edges

BITS = (1, 2, 3, 4, 8)
F32 = np.float32


@pytest.mark.parametrize("bits", BITS)
def test_the_special_ranges(bits):
    qmax = F32(2 ** bits - 1)
    x = np.array([[-3.0, -1.5, -0.25]], F32)              # all negative: extended to 0, the zero point is qmax
    s, z, inv, pad = am.qparams(x, bits)[0]
    assert s == F32(3.0) / qmax and inv == F32(1) / s and z == qmax and pad == 0
    x = np.array([[0.5, 2.0, 7.0]], F32)                  # all positive: lo = 0, the zero point is 0
    s, z, inv, _ = am.qparams(x, bits)[0]
    assert s == F32(7.0) / qmax and z == 0 and not np.signbit(z)
    for x in (np.zeros((3, 4), F32), np.array([[-0.0, 0.0]], F32), np.array([[np.nan, np.inf, -np.inf]], F32)):
        qp = am.qparams(x, bits)                          # all zero, signed zeros, nothing finite: lo = hi = 0 -> scale 1
        assert qp.view(np.uint32).tolist() == np.array([[1, 0, 1, 0]], F32).view(np.uint32).tolist()
    x = np.full((5, 2), 2.5, F32)                         # constant: the range is [0, 2.5]
    s, z, _, _ = am.qparams(x, bits)[0]
    assert s == F32(2.5) / qmax and z == 0
    x = np.array([[np.nan, -2.0, np.inf, 6.0, -np.inf]], F32)    # NaN and infinities do not count
    s, z, inv, _ = am.qparams(x, bits)[0]
    assert s == F32(8.0) / qmax and z == np.rint(F32(2.0) * inv)
    q = am.quantise(x, am.qparams(x, bits), bits)[0]
    assert q[0] == z and q[2] == qmax and q[4] == 0 and q[1] == 0 and q[3] == qmax
    tiny = F32(2.0 ** -110)                               # hi - lo below 2^-100: the scale's floor
    s, z, inv, _ = am.qparams(np.array([[0.0, tiny]], F32), bits)[0]
    assert s == F32(2.0 ** -100) and inv == F32(2.0 ** 100) and z == 0
    s, z, _, _ = am.qparams(np.array([[-tiny, 0.0]], F32), bits)[0]
    assert s == F32(2.0 ** -100) and z == 0               # rint(2^-10) = 0


def test_per_column_groups_are_the_columns():
    rng = np.random.default_rng(0)
    x = rng.normal(size=(33, 5)).astype(F32) * np.array([1, 4, 0, 0.01, 100], F32)
    x[3, 1] = np.nan
    qp = am.qparams(x, 4, per_column=True)
    assert qp.shape == (5, 4)
    for c in range(5):
        assert qp[c].tobytes() == am.qparams(x[:, c:c + 1], 4)[0].tobytes()
    q = am.quantise(x, qp, 4)
    for c in range(5):
        assert (q[:, c] == am.quantise(x[:, c:c + 1], qp[c:c + 1], 4)[:, 0]).all()


@pytest.mark.parametrize("bits", (2, 4, 8))
def test_ties_round_to_even(bits):
    qmax = 2 ** bits - 1
    zq = qmax // 2
    x = am.tie_inputs(bits)
    qp = am.qparams(x, bits)
    assert qp[0, 0] == 2 and qp[0, 2] == 0.5 and qp[0, 1] == zq
    q = am.quantise(x, qp, bits)[0]
    assert x.shape[1] == 2 + qmax and (x[0, 2:] % 2 == 1).all()
    # v / 2 = k + 0.5 goes to the even one of k, k + 1 (Python's round is half-to-even on exact halves)
    assert q.tolist() == [0, qmax] + [round(float(v) / 2) + zq for v in x[0, 2:]]
    assert len(set((q[2:] - zq) % 2)) == 1
    assert np.rint(F32(0.5)) == 0 and np.rint(F32(1.5)) == 2 and np.rint(F32(2.5)) == 2 and np.rint(F32(-0.5)) == 0   # half to even


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("seed", range(4))
def test_the_zero_point_and_the_half_step_bound(bits, seed):
    rng = np.random.default_rng(100 * bits + seed)
    shift = (0.0, 3.0, -3.0, 0.3)[seed]
    x = (rng.normal(size=(40, 9)) * 10.0 ** rng.integers(-3, 4) + shift).astype(F32)
    for per_column in (False, True):
        qp = am.qparams(x, bits, per_column)
        z = qp[:, 1]
        assert (z == np.rint(z)).all() and (z >= 0).all() and (z <= 2 ** bits - 1).all() and not np.signbit(z).any()
        q = am.quantise(x, qp, bits)
        assert q.min() >= 0 and q.max() <= 2 ** bits - 1
        assert (am.quantise(np.zeros_like(x), qp, bits) == z.astype(np.int32)[None, :]).all()       # 0.0 is represented exactly
        s = qp[:, 0].astype(np.float64)[None, :]
        back = s * (q.astype(np.float64) - z.astype(np.float64)[None, :])
        assert (np.abs(x.astype(np.float64) - back) <= am.HALF_STEP * s).all()


@pytest.mark.parametrize("a_bits,w_bits", [(8, 8), (8, 4), (4, 2), (1, 1)])
@pytest.mark.parametrize("per_column", [True, False])
def test_the_integer_identity(a_bits, w_bits, per_column):
    rng = np.random.default_rng(7)
    X, W = rng.normal(size=(33, 20)).astype(F32) + F32(0.5), rng.normal(size=(20, 7)).astype(F32)
    qa, cx, qb, cw, acc = am.linear_parts(X, W, a_bits, w_bits, per_column)
    t = am.dequant_t(acc, 20, qa, am.sums(cx, False), qb, am.sums(cw, True))
    za, zb = int(qa[0, 1]), np.broadcast_to(qb[:, 1].astype(np.int64), (7,))
    assert (t == (cx.astype(np.int64) - za) @ (cw.astype(np.int64) - zb[None, :])).all()
    # the int64 matters: K za zb beyond 2^31
    big = am.dequant_t(np.full((1, 1), 2.0 ** 24 - 1, F32), 2 ** 31 - 1, np.array([[1, 255, 1, 0]], F32), None, np.array([[1, 255, 1, 0]], F32), None)
    assert int(big[0, 0]) == 2 ** 24 - 1 + (2 ** 31 - 1) * 255 * 255


@pytest.mark.parametrize("a_bits,w_bits", [(8, 8), (8, 4), (4, 2), (1, 1)])
@pytest.mark.parametrize("per_column", [True, False])
def test_the_bound_of_linear(a_bits, w_bits, per_column):
    rng = np.random.default_rng(11)
    worst = 0.0
    for M, K, N in ((1, 1, 1), (33, 20, 7), (100, 130, 64)):
        X, W = rng.normal(size=(M, K)).astype(F32), rng.normal(size=(K, N)).astype(F32)
        qa, _, qb, _, _ = am.linear_parts(X, W, a_bits, w_bits, per_column)
        got = am.linear(X, W, a_bits, w_bits, per_column)
        err = np.abs(got.astype(np.float64) - X.astype(np.float64) @ W.astype(np.float64))
        bound = am.linear_bound(X, W, qa, qb, got)
        assert (err <= bound).all()
        worst = max(worst, float((err / bound).max()))
    print(f"linear a{a_bits} w{w_bits} per_column={per_column}: worst error / bound {worst:.3f}")


def _graph(n, seed):
    src, dst = random_edges(np.random.default_rng(seed), n, 3 * n)
    return src, dst


@pytest.mark.parametrize("bits", (2, 8))
@pytest.mark.parametrize("transposed", [False, True])
def test_the_bound_of_aggregate(bits, transposed):
    n = 100
    A = am.dense_view(*_graph(n, 3), n, transposed)
    rng = np.random.default_rng(5)
    T = rng.normal(size=(n, 5)).astype(F32)
    R, S = rng.random(n) < 0.5, rng.random(n) < 0.5
    qt = am.qparams(T, bits)
    for scale, (rm, sm) in ((None, (None, None)), (am.inv_degree(A.sum(axis=1)), (None, None)), (None, (R, S))):
        got = am.aggregate(A, T, bits, scale, rm, sm)
        Am = am.masked_view(A, rm, sm)
        exact = Am.astype(np.float64) @ T.astype(np.float64)
        if scale is not None:
            exact = exact * scale.astype(np.float64)[:, None]
        assert (np.abs(got - exact) <= am.aggregate_bound(Am, qt, got, scale)).all()
        dead = Am.sum(axis=1) == 0
        assert dead.any() and (got[dead].view(np.uint32) == 0).all()          # no live neighbour: +0


def test_per_column_weights_are_no_worse_on_columns_of_different_scale():
    """W's columns differ in scale by up to 2^6. Not a theorem for one draw: seed 0 was tried first and holds (the per-column errors of
    the seven columns are 0.06 - 0.11 each, the per-tensor ones fall from 1.0 on the smallest column to 0.09 on the largest)."""
    rng = np.random.default_rng(0)
    X = rng.normal(size=(100, 32)).astype(F32)
    W = (rng.normal(size=(32, 7)) * 2.0 ** np.arange(0, 7)).astype(F32)
    exact = X.astype(np.float64) @ W.astype(np.float64)
    col = np.linalg.norm(am.linear(X, W, 8, 4, True) - exact, axis=0) / np.linalg.norm(exact, axis=0)
    ten = np.linalg.norm(am.linear(X, W, 8, 4, False) - exact, axis=0) / np.linalg.norm(exact, axis=0)
    print("per column", col, "per tensor", ten)
    assert am.rel_error(am.linear(X, W, 8, 4, True), exact) <= am.rel_error(am.linear(X, W, 8, 4, False), exact)
    assert col[0] < ten[0] / 4        # the smallest column is where the per-tensor step hurts


COMPOSITION = dict(n=300, F=24, H=32, C=7, seed=0)


def composition(bits, norm, n=300, F=24, H=32, C=7, seed=0):
    rng = np.random.default_rng(seed)
    A = am.dense_view(*_graph(n, seed + 1), n)
    X, W_in, W_out = (rng.normal(size=s).astype(F32) for s in ((n, F), (F, H), (H, C)))
    return am.rel_error(am.gcn(A, X, W_in, W_out, bits, bits, norm), am.gcn_f64(A, X, W_in, W_out, norm))


@pytest.mark.parametrize("norm", [None, "mean", "sym"])
def test_the_composition_improves_with_the_bit_width(norm):
    """linear -> aggregate -> linear -> aggregate at n = 300, dims 24 / 32 / 7, Gaussian X and W, seed 0 (the seed holds the ordering;
    the errors at 8 bits are a few per cent, at 4 bits a few tens)."""
    e4, e6, e8 = (composition(b, norm, **COMPOSITION) for b in (4, 6, 8))
    print(f"norm={norm}: relative error 4 bits {e4:.4f}, 6 bits {e6:.4f}, 8 bits {e8:.4f}")
    assert e8 < e6 < e4 and e8 < 0.05
