"""The NumPy model of the edge softmax (tests/tiled_esoftmax_model.py) against its float64 definition, against deliberately wrong
variants and against the attention model: what the device is compared with bit for bit must itself be right, and the test inputs must
be able to tell a wrong rule from the contract. Graphs: those of tests/test_tiled_edge_gpu.py. No GPU.

The bounds. alpha: the logit difference is one rounding, EXP is within 2 ulp of exp for z <= 0 and exp'(z) <= 1, the d-term fold of
positive terms adds at most d - 1 roundings to den, the division and the final product one each: relative error below
(d + 8) * 2^-23 with d the owner's number of cells. The gradient: with sum(alpha) = 1, S is a d-term fold of terms bounded by
alpha_k * max|g|, so |S - exact| <= (d + 1) * 2^-24 * max|g|; the difference and the product add two roundings of values bounded by
2 max|g| and alpha <= 1: absolute error below (d + 16) * 2^-23 * max|g| (alpha is the same float32 vector on both sides)."""
import functools

import numpy as np
import pytest

import tiled_attn_model as am
import tiled_edge_model as em
import tiled_esoftmax_model as sm

NS = (1, 33, 129, 300)
EPS = 2.0 ** -23


@functools.lru_cache(maxsize=None)
def case(n):
    src, dst = sm.graph_edges(n)
    nnz = em.slot_cells(src, dst, n)[0].size
    rng = np.random.default_rng(7 * n + 1)
    logits = (3 * rng.normal(size=nnz)).astype(np.float32)
    g = rng.normal(size=nnz).astype(np.float32)
    return src, dst, nnz, logits, g


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_the_graphs_have_the_hard_cases():
    src, dst, nnz, _, _ = case(300)
    row, col = em.slot_cells(src, dst, 300)
    rdeg, cdeg = np.bincount(row, minlength=300), np.bincount(col, minlength=300)
    assert cdeg[7] >= 290, "a hub column"
    assert (rdeg[32:64] >= 128).all(), "a full tile"
    assert rdeg[5] == 0 and cdeg[9] == 0, "an empty row and an empty column"
    assert case(1)[2] >= 0 and case(33)[2] > 0 and case(129)[2] > 0


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("n", NS)
def test_forward_is_within_its_bound_of_float64(n, transposed):
    src, dst, nnz, logits, _ = case(n)
    alpha, m, inv = sm.edge_softmax_f32(src, dst, n, logits, transposed)
    want = sm.edge_softmax_f64(src, dst, n, logits, transposed)
    deg = sm.owner_degree_per_slot(src, dst, n, transposed)
    rel = np.abs(alpha.astype(np.float64) - want) / want if nnz else np.zeros(0)
    print(f"n={n} T={transposed}: max relative error {rel.max() if nnz else 0:.3g}")
    assert (rel <= (deg + 8) * EPS).all()
    # the statistics: m is the owner's largest logit, inv the reciprocal of a sum that is at least 1; none for an owner without cells
    owner, _, slot, odeg = sm.owner_lists(src, dst, n, transposed)
    mx = np.full(n, -np.inf, dtype=np.float32)
    np.maximum.at(mx, owner, logits[slot])
    assert np.array_equal(m[odeg > 0], mx[odeg > 0]) and (bits(m[odeg == 0]) == 0).all() and (bits(inv[odeg == 0]) == 0).all()
    assert ((inv[odeg > 0] > 0) & (inv[odeg > 0] <= 1)).all()
    sums = np.bincount(owner, weights=alpha[slot].astype(np.float64), minlength=n)
    assert np.allclose(sums[odeg > 0], 1.0, atol=(odeg.max() + 8) * EPS)


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("n", NS)
def test_gradient_is_within_its_bound_of_float64(n, transposed):
    src, dst, nnz, logits, g = case(n)
    alpha, _, _ = sm.edge_softmax_f32(src, dst, n, logits, transposed)
    got = sm.edge_softmax_grad_f32(src, dst, n, alpha, g, transposed)
    want = sm.edge_softmax_grad_f64(src, dst, n, alpha, g, transposed)
    deg = sm.owner_degree_per_slot(src, dst, n, transposed)
    err = np.abs(got.astype(np.float64) - want)
    gmax = float(np.abs(g).max()) if nnz else 0.0
    print(f"n={n} T={transposed}: max absolute error {err.max() if nnz else 0:.3g}")
    assert (err <= (deg + 16) * EPS * gmax).all()


def test_gradient_is_the_derivative():
    """central differences of the float64 softmax agree with the float64 gradient formula the model is held against"""
    n = 33
    src, dst, nnz, logits, g = case(n)
    for transposed in (False, True):
        l64 = logits.astype(np.float64)
        a64 = sm.edge_softmax_f64(src, dst, n, l64, transposed)
        want = sm.edge_softmax_grad_f64(src, dst, n, a64, g, transposed)
        h = 1e-6
        for k in range(0, nnz, max(1, nnz // 12)):
            e = np.zeros(nnz)
            e[k] = h
            num = ((sm.edge_softmax_f64(src, dst, n, l64 + e, transposed) - sm.edge_softmax_f64(src, dst, n, l64 - e, transposed)) * g).sum() / (2 * h)
            assert abs(num - want[k]) < 1e-7


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("n", [33, 129, 300])
def test_wrong_variants_differ(n, transposed):
    src, dst, nnz, logits, g = case(n)
    alpha, m, inv = sm.edge_softmax_f32(src, dst, n, logits, transposed)
    for wrong in sm.FORWARD_WRONG:
        a2, m2, inv2 = sm.edge_softmax_f32(src, dst, n, logits, transposed, wrong=wrong)
        assert np.array_equal(m2, m)
        assert (bits(a2) != bits(alpha)).any(), wrong
        if wrong == "descending":
            print(f"n={n} T={transposed}: descending changes inv on {(bits(inv2) != bits(inv)).sum()} owners")
            assert (bits(inv2) != bits(inv)).any()
    ref = sm.edge_softmax_grad_f32(src, dst, n, alpha, g, transposed)
    for wrong in sm.GRAD_WRONG:
        assert (bits(sm.edge_softmax_grad_f32(src, dst, n, alpha, g, transposed, wrong=wrong)) != bits(ref)).any(), wrong


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("n", NS)
def test_statistics_equal_the_attention_models(n, transposed):
    src, dst, nnz, _, _ = case(n)
    rng = np.random.default_rng(n + 11)
    p, q = rng.normal(size=n).astype(np.float32), rng.normal(size=n).astype(np.float32)
    X = rng.normal(size=(n, 3)).astype(np.float32)
    _, m_att, inv_att = am.attention_f32(src, dst, n, X, p, q, 0.2, transposed)
    logits = sm.pair_logits(src, dst, n, p, q, 0.2, transposed)
    alpha, m, inv = sm.edge_softmax_f32(src, dst, n, logits, transposed)
    deg = sm.owner_lists(src, dst, n, transposed)[3]
    assert np.array_equal(bits(inv), bits(inv_att))
    assert np.array_equal(bits(m[deg > 0]), bits(m_att[deg > 0]))
    # and the weights give the attention's output when they weigh the sum term by term (the attention scales the finished sum instead,
    # so only closeness is due)
    Y = em.weighted_f32(src, dst, n, X, alpha, transposed)
    assert np.allclose(Y, am.attention_f32(src, dst, n, X, p, q, 0.2, transposed)[0], rtol=1e-5, atol=1e-5)


def test_a_minus_infinity_masks_its_edge():
    n = 129
    src, dst, nnz, logits, _ = case(n)
    for transposed in (False, True):
        owner, _, slot, deg = sm.owner_lists(src, dst, n, transposed)
        start = np.concatenate([[0], np.cumsum(deg)[:-1]])
        big = np.flatnonzero(deg >= 2)
        masked = slot[start[big]]                      # the first cell of every owner with two or more
        l2 = logits.copy()
        l2[masked] = -np.inf
        alpha, m, inv = sm.edge_softmax_f32(src, dst, n, l2, transposed)
        assert (bits(alpha[masked]) == 0).all()
        # the other cells: the softmax of the graph without the masked ones
        keep = np.ones(nnz, dtype=bool)
        keep[masked] = False
        want = sm.edge_softmax_f64(src, dst, n, np.where(keep, l2, -1e30), transposed)
        assert np.allclose(alpha[keep], want[keep], rtol=(deg.max() + 8) * EPS, atol=0)
        assert np.isfinite(alpha).all() and np.isfinite(m).all() and np.isfinite(inv).all()


def test_the_composed_attention_is_dense_attention():
    n, d, N = 129, 16, 5
    src, dst, nnz, _, _ = case(n)
    rng = np.random.default_rng(5)
    Q, K = rng.normal(size=(n, d)).astype(np.float32), rng.normal(size=(n, d)).astype(np.float32)
    V, dY = rng.normal(size=(n, N)).astype(np.float32), rng.normal(size=(n, N)).astype(np.float32)
    row, col = em.slot_cells(src, dst, n)
    for transposed in (False, True):
        A = np.zeros((n, n), dtype=bool)
        A[(col, row) if transposed else (row, col)] = True
        S = np.where(A, Q.astype(np.float64) @ K.astype(np.float64).T * 0.25, -np.inf)
        with np.errstate(invalid="ignore"):
            P = np.exp(S - S.max(axis=1, keepdims=True))
            P = np.nan_to_num(P / P.sum(axis=1, keepdims=True))
        out, _, _ = sm.edge_attention_f32(src, dst, n, Q, K, V, 0.25, transposed)
        assert np.allclose(out, P @ V, rtol=1e-4, atol=1e-5)
        # the gradients, against the dense formulas
        dQ, dK, dV = sm.edge_attention_grads_f32(src, dst, n, Q, K, V, 0.25, dY, transposed)
        dP = dY.astype(np.float64) @ V.astype(np.float64).T
        dS = P * (dP - (P * dP).sum(axis=1, keepdims=True)) * 0.25
        assert np.allclose(dV, P.T @ dY, rtol=1e-4, atol=1e-5)
        assert np.allclose(dQ, dS @ K, rtol=1e-4, atol=1e-5) and np.allclose(dK, dS.T @ Q, rtol=1e-4, atol=1e-5)
