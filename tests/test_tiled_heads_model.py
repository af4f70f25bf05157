"""The multi-head models (tests/tiled_heads_model.py) against a dense float64 multi-head attention with torch's autograd, on small
graphs: what the device is compared with bit for bit must itself be right. The tolerance is the one tests/test_transformer_reference.py
uses for one head, layers_reference.tolerances: 8 . max(max|T_f32 - T_f64|, 2^-24 . max|T_f64|) from the dense reference alone. No GPU."""
import functools

import numpy as np
import pytest
import torch

import layers_reference as R
import tiled_edge_model as em
import tiled_esoftmax_model as sm
import tiled_heads_model as hm

NS = (33, 129)
SHAPES = ((1, 5), (3, 5), (8, 8), (2, 48))
VIEWS = (False, True)


@functools.lru_cache(maxsize=None)
def case(n, heads, d):
    src, dst = sm.graph_edges(n)
    rng = np.random.default_rng([n, heads, d])
    Q, K, V, dY = (rng.standard_normal((n, heads * d)).astype(np.float32) for _ in range(4))
    return src, dst, Q, K, V, dY


def dense_attention(src, dst, n, Q, K, V, dY, heads, transposed, dtype):
    """{"Y", "dQ", "dK", "dV"}: per head softmax over the view's neighbours of q_i . k_j . float32(1 / sqrt(d)), times v_j; a row
    without neighbours gives 0"""
    row, col = em.slot_cells(src, dst, n)
    m = np.zeros((n, n), dtype=bool)
    m[(col, row) if transposed else (row, col)] = True
    m = torch.from_numpy(m)
    Q, K, V = (torch.as_tensor(t, dtype=dtype).clone().requires_grad_(True) for t in (Q, K, V))
    d = Q.shape[1] // heads
    scale = torch.tensor(1.0 / np.sqrt(d), dtype=torch.float64).to(torch.float32).to(dtype)   # the call multiplies by a float32
    has = m.any(dim=1, keepdim=True)
    outs = []
    for h in range(heads):
        c = hm.head_cols(h, d)
        S = (Q[:, c] @ K[:, c].T) * scale
        top = torch.where(has, S.masked_fill(~m, float("-inf")).max(dim=1, keepdim=True).values, torch.zeros((), dtype=dtype)).detach()
        w = torch.where(m, torch.exp(S - top), torch.zeros((), dtype=dtype))
        den = w.sum(dim=1, keepdim=True)
        outs.append((w / torch.where(has, den, torch.ones_like(den))) @ V[:, c])
    Y = torch.cat(outs, dim=1)
    dQ, dK, dV = torch.autograd.grad(Y, (Q, K, V), torch.as_tensor(dY, dtype=dtype))
    return {"Y": Y.detach(), "dQ": dQ, "dK": dK, "dV": dV}


@pytest.mark.parametrize("transposed", VIEWS)
@pytest.mark.parametrize("heads,d", SHAPES)
@pytest.mark.parametrize("n", NS)
def test_attention_and_gradients_are_within_the_tolerance_of_float64(n, heads, d, transposed):
    src, dst, Q, K, V, dY = case(n, heads, d)
    ref64 = dense_attention(src, dst, n, Q, K, V, dY, heads, transposed, torch.float64)
    ref32 = dense_attention(src, dst, n, Q, K, V, dY, heads, transposed, torch.float32)
    tol = R.tolerances(ref64, ref32)
    dQ, dK, dV = hm.edge_attention_grads_heads_f32(src, dst, n, Q, K, V, heads, dY, transposed=transposed)
    got = {"Y": hm.edge_attention_heads_f32(src, dst, n, Q, K, V, heads, transposed=transposed), "dQ": dQ, "dK": dK, "dV": dV}
    for name, want in ref64.items():
        assert got[name].dtype == np.float32 and got[name].shape == tuple(want.shape)
        err = float(np.abs(got[name].astype(np.float64) - want.numpy()).max())
        print(f"n={n} H={heads} d={d} T={transposed} {name}: error {err:.3e}, tolerance {tol[name]:.3e}")
        assert 0 < tol[name] and err <= tol[name], name


@pytest.mark.parametrize("transposed", VIEWS)
def test_the_pieces_are_the_single_head_models_on_slices(transposed):
    n, heads, d = 129, 3, 5
    src, dst, Q, K, V, _ = case(n, heads, d)
    s = hm.sddmm_heads_f32(src, dst, n, Q, K, heads, transposed)
    nnz = em.slot_cells(src, dst, n)[0].size
    assert s.shape == (nnz, heads) and s.flags.c_contiguous
    alpha, m, inv = hm.edge_softmax_heads_f32(src, dst, n, s, transposed)
    assert alpha.shape == (nnz, heads) and m.shape == (n, heads) and inv.shape == (n, heads)
    g = np.random.default_rng(5).standard_normal((nnz, heads)).astype(np.float32)
    dl = hm.edge_softmax_grad_heads_f32(src, dst, n, alpha, g, transposed)
    Y = hm.weighted_heads_f32(src, dst, n, V, alpha, transposed)
    for h in range(heads):
        c = hm.head_cols(h, d)
        np.testing.assert_array_equal(s[:, h].view(np.uint32), em.sddmm_f32(src, dst, n, Q[:, c], K[:, c], transposed).view(np.uint32))
        a1, m1, i1 = sm.edge_softmax_f32(src, dst, n, s[:, h], transposed)
        for got, want in ((alpha[:, h], a1), (m[:, h], m1), (inv[:, h], i1)):
            np.testing.assert_array_equal(np.ascontiguousarray(got).view(np.uint32), want.view(np.uint32))
        np.testing.assert_array_equal(np.ascontiguousarray(dl[:, h]).view(np.uint32),
                                      sm.edge_softmax_grad_f32(src, dst, n, a1, g[:, h], transposed).view(np.uint32))
        np.testing.assert_array_equal(np.ascontiguousarray(Y[:, c]).view(np.uint32),
                                      em.weighted_f32(src, dst, n, V[:, c], a1, transposed).view(np.uint32))
    # the softmax of every head sums to one over an owner with cells, and the heads differ
    owner = em.slot_cells(src, dst, n)[1 if transposed else 0]
    sums = np.zeros((n, heads))
    np.add.at(sums, owner, alpha.astype(np.float64))
    assert np.allclose(sums[np.bincount(owner, minlength=n) > 0], 1.0, atol=1e-5)
    assert not np.array_equal(alpha[:, 0], alpha[:, 1])


def test_the_shapes_reach_every_route_of_the_per_edge_dot():
    routes = {hm.sddmm_heads_variant(H * d, H) for H, d in hm.HEAD_SHAPES + hm.SDDMM_MORE_SHAPES}
    assert routes == {("narrow", 1), ("narrow", 2), ("narrow", 4), ("narrow", 0), ("wide", 4), ("wide", 6), ("wide", 0)}
    assert hm.sddmm_heads_variant(320, 5) == ("narrow", 0) and hm.sddmm_heads_variant(320, 40) == ("narrow", 0)
    assert hm.sddmm_heads_variant(64, 8) == ("narrow", 1) and hm.sddmm_heads_variant(200, 2) == ("wide", 4)
