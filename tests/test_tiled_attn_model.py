"""The model of the attention tiled products (tests/tiled_attn_model.py) against float64: EXP and DOT against their real values, the
forward and the three gradients against a dense float64 masked softmax differentiated by torch.autograd, and the proof that the test
inputs tell deliberately wrong rules from the contract. No GPU."""
import math

import numpy as np
import pytest

from tiled_attn_model import attention_f32, attention_grads_f32, dot_f32, exp_f32, lrelu_f32
from tiled_float_model import neighbour_lists
from tiled_model import random_edges, set_cells

U = 2.0 ** -24      # the unit roundoff of float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1. EXP ---------------------------------------------------------------------------------------------------------------------------
def _exp_sample():
    """A fixed sample of [-87, 0]: both ends, 4096 points of every binade from 2^-149 up to 64 .. 87 (evenly spaced, ends included),
    and the neighbours of every multiple of ln 2 / 2, where the reduction's k changes."""
    parts = [np.array([-87.0, -0.0, 0.0], dtype=np.float32)]
    for ex in range(-149, 7):
        lo, hi = 2.0 ** ex, min(2.0 ** (ex + 1), 87.0)
        parts.append(-np.linspace(lo, hi, 4096).astype(np.float32))
    half = (-np.arange(1, 252) * (math.log(2.0) / 2)).astype(np.float32)
    half = half[half >= -87]
    parts += [half, np.nextafter(half, np.float32(0)), np.nextafter(half, np.float32(-100))]
    z = np.concatenate(parts)
    return z[z >= -87]


def test_exp_is_within_two_ulp_of_the_real_exponential():
    z = _exp_sample()
    assert z.min() == -87 and z.max() == 0 and z.size > 600000
    exps = np.frexp(z[z < 0])[1]
    assert set(range(-148, 8)) <= set(exps.tolist())          # every exponent of the arguments down to the subnormals
    w = exp_f32(z)
    assert w.dtype == np.float32
    want = np.exp(z.astype(np.float64))
    ulp = np.spacing(want.astype(np.float32)).astype(np.float64)
    err = np.abs(w.astype(np.float64) - want) / ulp
    print(f"EXP: worst error {err.max():.3f} ulp over {z.size} arguments")
    assert err.max() <= 2.0
    tiny = float(np.finfo(np.float32).tiny)
    assert w.min() >= tiny and w.max() == 1.0                 # normal numbers in [FLT_MIN, 1]: no subnormal is produced


def test_exp_at_its_ends():
    assert _bits(exp_f32(np.float32(0.0))) == 0x3F800000 and _bits(exp_f32(np.float32(-0.0))) == 0x3F800000
    below = np.array([np.nextafter(np.float32(-87), np.float32(-100)), -88, -100, -1e30, -np.inf], dtype=np.float32)
    assert (_bits(exp_f32(below)) == 0).all()
    assert exp_f32(np.float32(-87.0)) > 0
    z = _exp_sample()
    z = np.sort(z)
    assert (np.diff(exp_f32(z).astype(np.float64)) >= -2 * np.spacing(exp_f32(z[1:]))).all()    # monotone up to its error


# ---- 2. DOT ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 16, 63, 64, 65, 129, 257, 600])
def test_dot_against_float64(N):
    rng = np.random.default_rng(N)
    x, y = rng.standard_normal((50, N)).astype(np.float32), rng.standard_normal((50, N)).astype(np.float32)
    got = dot_f32(x, y)
    terms = x.astype(np.float64) * y.astype(np.float64)
    # a term is rounded once as a product and takes part in at most ceil(N / 64) + 6 adds
    tol = (math.ceil(N / 64) + 7) * U * np.abs(terms).sum(axis=1)
    assert (np.abs(got.astype(np.float64) - terms.sum(axis=1)) <= tol).all()
    if N == 1:
        assert (_bits(got) == _bits(x[:, 0] * y[:, 0])).all()
    assert (_bits(dot_f32(y, x)) == _bits(got)).all()          # commutative, word for word
    if N > 64:                                                 # up to 64 columns a lane adds one product to +0: nothing to fuse
        assert (_bits(dot_f32(x, y, fma=True)) != _bits(got)).any()


# ---- 3. forward and gradients against a dense float64 reference ---------------------------------------------------------------------------
def _dense_reference(src, dst, n, X, p, q, slope, dY, transposed):
    """float64 masked softmax on the dense adjacency, differentiated by torch.autograd: Y, dX, dp, dq and alpha."""
    import torch

    cells = set_cells(src, dst, n)
    A = np.zeros((n, n), bool)
    A[cells // n, cells % n] = True
    A = torch.from_numpy(A.T.copy() if transposed else A)
    Xt, pt, qt = (torch.from_numpy(np.asarray(t, dtype=np.float64)).requires_grad_(True) for t in (X, p, q))
    logits = torch.nn.functional.leaky_relu(pt[:, None] + qt[None, :], slope)
    logits = torch.where(A, logits, torch.full((), -float("inf"), dtype=torch.float64))
    alpha = torch.softmax(logits, dim=1)
    alpha = torch.where(A.any(dim=1)[:, None], alpha, torch.zeros((), dtype=torch.float64))
    Y = alpha @ Xt
    Y.backward(torch.from_numpy(np.asarray(dY, dtype=np.float64)))
    return Y.detach().numpy(), Xt.grad.numpy(), pt.grad.numpy(), qt.grad.numpy(), alpha.detach().numpy()


@pytest.mark.parametrize("slope", [0.0, 0.2, 1.0])
@pytest.mark.parametrize("n,N", [(97, 17), (300, 70)])
def test_the_model_against_a_dense_float64_softmax(n, N, slope):
    """Scores in [-1, 1], so a logit and its shift are below 2 in magnitude and z = L(e) - m carries an absolute error below 12 u
    (u = 2^-24: e, L, m and the subtraction), EXP adds 2 ulp = 4 u and the reciprocal, the normalisation and the product with X one
    rounding each: fewer than 40 roundings per weight whatever the row. On top come the d adds of a fold and, in the score gradients,
    the ceil(N / 64) + 6 adds of DOT. Hence the bound (d_max + ceil(N / 64) + 40) u times the float64 sum of the absolute terms."""
    rng = np.random.default_rng(7 * n + N)
    src, dst = random_edges(rng, n, 6 * n + 5)
    keep = ~np.isin(src, (3, n - 1)) & ~np.isin(dst, (3, n - 1))      # two nodes without neighbours on either view
    src, dst = src[keep], dst[keep]
    X, dY = rng.standard_normal((n, N)).astype(np.float32), rng.standard_normal((n, N)).astype(np.float32)
    p, q = rng.uniform(-1, 1, n).astype(np.float32), rng.uniform(-1, 1, n).astype(np.float32)
    for transposed in (False, True):
        Y, m, inv = attention_f32(src, dst, n, X, p, q, slope, transposed)
        dX, dp, dq, D = attention_grads_f32(src, dst, n, X, p, q, dY, Y, m, inv, slope, transposed)
        rY, rdX, rdp, rdq, alpha = _dense_reference(src, dst, n, X, p, q, slope, dY, transposed)
        _, _, deg = neighbour_lists(src, dst, n, transposed)
        _, _, deg_other = neighbour_lists(src, dst, n, not transposed)
        d_max = int(max(deg.max(), deg_other.max()))
        bound = (d_max + math.ceil(N / 64) + 40) * U
        aX, adY = np.abs(X.astype(np.float64)), np.abs(dY.astype(np.float64))
        checks = {"Y": (Y, rY, alpha @ aX), "dX": (dX, rdX, alpha.T @ adY)}
        # u = alpha . (dY[o] . X[k] - dY[o] . Y[o]): the absolute terms of both dots, under alpha
        edge = alpha * (adY @ aX.T + (adY * (alpha @ aX)).sum(axis=1)[:, None])
        checks["dp"] = (dp, rdp, edge.sum(axis=1))
        checks["dq"] = (dq, rdq, edge.sum(axis=0))
        for name, (got, want, mag) in checks.items():
            err = np.abs(got.astype(np.float64) - want)
            worst = float((err / np.maximum(bound * mag, 1e-300)).max())
            print(f"n={n} N={N} slope={slope} transposed={transposed} {name}: worst error / bound = {worst:.4f}")
            assert (err <= bound * mag).all(), (name, transposed, worst)
            assert np.abs(want).max() > 0
        empty = deg == 0
        assert empty.any() and (_bits(Y[empty]) == 0).all() and (_bits(inv[empty]) == 0).all()
        assert (_bits(m[empty]) == _bits(lrelu_f32(p[empty], slope))).all()
        assert (inv[~empty] <= 1).all() and (inv[~empty] > 0).all()       # den >= 1: the maximal neighbour weighs exactly 1


# ---- 4. wrong rules disagree ------------------------------------------------------------------------------------------------------------
def test_wrong_rules_disagree_with_the_model():
    """Scores on a grid of eighths, so that e = p[o] + q[k] is exactly 0 on many edges."""
    n, N = 300, 33
    rng = np.random.default_rng(11)
    src, dst = random_edges(rng, n, 6 * n + 5)
    X, dY = rng.standard_normal((n, N)).astype(np.float32), rng.standard_normal((n, N)).astype(np.float32)
    p, q = (rng.integers(-8, 9, n) / 8).astype(np.float32), (rng.integers(-8, 9, n) / 8).astype(np.float32)
    for transposed in (False, True):
        o, k, _ = neighbour_lists(src, dst, n, transposed)
        assert ((p[o] + q[k]) == 0).sum() > 20
        Y, m, inv = attention_f32(src, dst, n, X, p, q, 0.2, transposed)
        for wrong in ("descending", "fma", "normalise_terms"):
            Yw, mw, invw = attention_f32(src, dst, n, X, p, q, 0.2, transposed, wrong=wrong)
            assert (_bits(Yw) != _bits(Y)).any(), wrong
            assert (_bits(mw) == _bits(m)).all()                  # the shift is a maximum: no rule of these moves it
            assert np.abs(Yw - Y).max() < 1e-4                    # ... and all of them are the same softmax
        grads = attention_grads_f32(src, dst, n, X, p, q, dY, Y, m, inv, 0.2, transposed)
        for wrong, differ in (("descending", (0, 1, 2)), ("zero_is_positive", (1, 2))):
            gw = attention_grads_f32(src, dst, n, X, p, q, dY, Y, m, inv, 0.2, transposed, wrong=wrong)
            for i in differ:
                assert (_bits(gw[i]) != _bits(grads[i])).any(), (wrong, i)
        # slope 1 makes L the identity: there the rule at e == 0 cannot matter
        Y1, m1, inv1 = attention_f32(src, dst, n, X, p, q, 1.0, transposed)
        g1 = attention_grads_f32(src, dst, n, X, p, q, dY, Y1, m1, inv1, 1.0, transposed)
        w1 = attention_grads_f32(src, dst, n, X, p, q, dY, Y1, m1, inv1, 1.0, transposed, wrong="zero_is_positive")
        assert all((_bits(a) == _bits(b)).all() for a, b in zip(g1, w1))


def test_masking_and_wide_spreads():
    """-inf masks a neighbour exactly; a spread of scores beyond 87 gives weights of exactly 0 and no NaN."""
    n, N = 200, 9
    rng = np.random.default_rng(3)
    src, dst = random_edges(rng, n, 8 * n)
    X = rng.standard_normal((n, N)).astype(np.float32)
    p, q = rng.uniform(-1, 1, n).astype(np.float32), rng.uniform(-1, 1, n).astype(np.float32)
    masked = rng.random(n) < 0.3
    qm = np.where(masked, -np.inf, q).astype(np.float32)
    o, k, deg = neighbour_lists(src, dst, n)
    alive = np.bincount(o[~masked[k]], minlength=n) > 0
    Y, m, inv = attention_f32(src, dst, n, X, p, qm, 0.2)
    cells = set_cells(src, dst, n)
    r, c = cells // n, cells % n
    sel = ~masked[c]
    Yk, mk, invk = attention_f32(r[sel], c[sel], n, X, p, q, 0.2)
    assert alive.sum() > n // 2
    assert (_bits(Y[alive]) == _bits(Yk[alive])).all() and (_bits(inv[alive]) == _bits(invk[alive])).all()
    wide = (rng.uniform(-1, 1, n) * 200).astype(np.float32)
    Yw, mw, invw = attention_f32(src, dst, n, X, p, wide, 0.2)
    assert np.isfinite(Yw).all() and (invw[deg > 0] <= 1).all()
    e = p[o] + wide[k]
    assert ((lrelu_f32(e, 0.2) - mw[o]) < -87).sum() > n
