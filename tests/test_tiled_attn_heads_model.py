"""The model of the attention tiled products with heads (tests/tiled_attn_heads_model.py, which is tests/tiled_attn_model.py per head)
against a dense float64 masked softmax differentiated by torch.autograd, per head; the proof that the test inputs tell a deliberately
wrong rule - head h reading head h + 1's scores - from the contract; and the hand-kept copy of the launchers' choices. No GPU."""
import math

import numpy as np
import pytest

import tiled_attn_heads_model as hm
from test_tiled_attn_model import U, _bits, _dense_reference
from tiled_float_model import neighbour_lists
from tiled_model import random_edges

N_NODES = 97


def _graph(rng, n):
    src, dst = random_edges(rng, n, 6 * n + 5)
    keep = ~np.isin(src, (3, n - 1)) & ~np.isin(dst, (3, n - 1))      # two nodes without neighbours on either view
    return src[keep], dst[keep]


@pytest.mark.parametrize("slope", [0.0, 0.2, 1.0])
@pytest.mark.parametrize("H,d", [(3, 5), (2, 65)])
def test_the_model_against_a_dense_float64_softmax_per_head(H, d, slope):
    """The bound is the single-head model's with N = d: scores in [-1, 1], fewer than 40 roundings per
    weight, the d_max adds of a fold and the ceil(d / 64) + 6 adds of a head's DOT - (d_max + ceil(d / 64) + 40) u times the float64
    sum of the absolute terms, head by head."""
    n = N_NODES
    rng = np.random.default_rng([n, H, d])
    src, dst = _graph(rng, n)
    X, dY = rng.standard_normal((n, H * d)).astype(np.float32), rng.standard_normal((n, H * d)).astype(np.float32)
    p, q = rng.uniform(-1, 1, (n, H)).astype(np.float32), rng.uniform(-1, 1, (n, H)).astype(np.float32)
    for transposed in (False, True):
        Y, m, inv = hm.attention_heads_f32(src, dst, n, X, p, q, slope, transposed)
        dX, dp, dq, D = hm.attention_grads_heads_f32(src, dst, n, X, p, q, dY, Y, m, inv, slope, transposed)
        assert Y.shape == (n, H * d) and m.shape == inv.shape == dp.shape == dq.shape == D.shape == (n, H)
        _, _, deg = neighbour_lists(src, dst, n, transposed)
        _, _, deg_other = neighbour_lists(src, dst, n, not transposed)
        d_max = int(max(deg.max(), deg_other.max()))
        bound = (d_max + math.ceil(d / 64) + 40) * U
        for h in range(H):
            cols = slice(h * d, (h + 1) * d)
            rY, rdX, rdp, rdq, alpha = _dense_reference(src, dst, n, X[:, cols], p[:, h], q[:, h], slope, dY[:, cols], transposed)
            aX, adY = np.abs(X[:, cols].astype(np.float64)), np.abs(dY[:, cols].astype(np.float64))
            edge = alpha * (adY @ aX.T + (adY * (alpha @ aX)).sum(axis=1)[:, None])
            checks = {"Y": (Y[:, cols], rY, alpha @ aX), "dX": (dX[:, cols], rdX, alpha.T @ adY),
                      "dp": (dp[:, h], rdp, edge.sum(axis=1)), "dq": (dq[:, h], rdq, edge.sum(axis=0))}
            for name, (got, want, mag) in checks.items():
                err = np.abs(got.astype(np.float64) - want)
                worst = float((err / np.maximum(bound * mag, 1e-300)).max())
                print(f"H={H} d={d} slope={slope} transposed={transposed} head {h} {name}: worst error / bound = {worst:.4f}")
                assert (err <= bound * mag).all(), (name, h, transposed, worst)
                assert np.abs(want).max() > 0
            assert (_bits(D[:, h]) == _bits(hm.dot_f32(dY[:, cols], Y[:, cols]))).all()
        empty = deg == 0
        assert empty.sum() >= 2
        assert (_bits(Y[empty]) == 0).all() and (_bits(inv[empty]) == 0).all() and (_bits(dp[empty]) == 0).all()


@pytest.mark.parametrize("H,d", [(3, 5), (2, 65)])
def test_a_head_reading_its_neighbours_scores_is_told_apart(H, d):
    n = N_NODES
    rng = np.random.default_rng([n, H, d, 1])
    src, dst = _graph(rng, n)
    X, dY = rng.standard_normal((n, H * d)).astype(np.float32), rng.standard_normal((n, H * d)).astype(np.float32)
    p, q = rng.uniform(-1, 1, (n, H)).astype(np.float32), rng.uniform(-1, 1, (n, H)).astype(np.float32)
    for transposed in (False, True):
        right = hm.attention_heads_f32(src, dst, n, X, p, q, 0.2, transposed)
        wrong = hm.attention_heads_f32(src, dst, n, X, p, q, 0.2, transposed, wrong="next_head")
        for name, r, w in zip(("Y", "m", "inv"), right, wrong):
            for h in range(H):
                cols = slice(h * d, (h + 1) * d) if name == "Y" else slice(h, h + 1)
                assert (_bits(r[:, cols]) != _bits(w[:, cols])).any(), (name, h)
        gr = hm.attention_grads_heads_f32(src, dst, n, X, p, q, dY, *right, 0.2, transposed)
        gw = hm.attention_grads_heads_f32(src, dst, n, X, p, q, dY, *right, 0.2, transposed, wrong="next_head")
        for name, r, w in zip(("dX", "dp", "dq"), gr, gw):
            assert (_bits(r) != _bits(w)).any(), name
        assert (_bits(gr[3]) == _bits(gw[3])).all()   # the row dot reads no score


def test_the_maximum_is_taken_per_column():
    n, H = N_NODES, 4
    rng = np.random.default_rng(5)
    src, dst = _graph(rng, n)
    q = rng.uniform(-1, 1, (n, H)).astype(np.float32)
    for transposed in (False, True):
        M = hm.max_heads_f32(src, dst, n, q, transposed)
        for h in range(H):
            assert (_bits(M[:, h]) == _bits(hm.max_heads_f32(src, dst, n, q[:, h:h + 1].copy(), transposed)[:, 0])).all()


def test_the_shapes_reach_every_variant():
    """The hand-kept copy of the launchers' switches: the issue's shapes reach both product tables, the narrow and the wide mapping of
    the score gradient and lanes whose columns straddle heads; the further shapes reach the remaining register classes."""
    shapes = hm.HEAD_SHAPES + hm.MORE_SHAPES
    for t in (False, True):
        assert {hm.product_variant(H, d, t) for H, d in hm.HEAD_SHAPES} == {(16, 1), (16, 4)}
        assert {hm.product_variant(H, d, t) for H, d in shapes} == set(hm.PRODUCT_VARIANTS)
        assert max(hm.product_chunks(H, d, t) for H, d in hm.HEAD_SHAPES) >= 2
        assert {hm.lanes_straddle_heads(H, d, t) for H, d in hm.HEAD_SHAPES} == {False, True}
    assert hm.product_variant(2, 1, False) == (16, 1) and hm.product_variant(64, 1, False) == (16, 4) and hm.product_variant(64, 1, True) == (16, 1)
    assert {hm.grad_variant(H, d)[0][0] for H, d in hm.HEAD_SHAPES} == {"narrow", "wide"}
    assert {hm.grad_variant(H, d)[0] for H, d in shapes} == set(hm.GRAD_VARIANTS)
    assert hm.grad_variant(12, 32) == (("narrow", 1), 6) and hm.grad_variant(2, 1) == (("narrow", 1), 1)
    assert hm.grad_variant(2, 33) == (("narrow", 1), 2) and hm.grad_variant(8, 8) == (("narrow", 1), 1)
    assert hm.grad_variant(2, 129) == (("wide", 4), 2) and hm.grad_variant(2, 257) == (("wide", 0), 2)
    # a lane never holds more columns than a head has on the column view: a chunk then touches at most 17 heads
    for H, d in shapes + ((64, 1), (40, 2), (30, 3)):
        lpr, cpl = hm.product_variant(H, d, True)
        assert cpl <= d and (lpr * cpl - 1) // d + 2 <= 17
