"""conv.TransformerConv on the device against the dense float64 definition of tests/transformer_reference.py, gradients for X, W_q, W_k
and W_v included. Every case runs the real layer on ``adj``, on ``adj.T`` and on both views of ``pack_edges_tiled(..., reorder=True)``
of the same edge list, with the parameters the reference used; X and the result are in the edge list's numbering and every element is
compared. Every tensor lies within the tolerance the reference computes for it, tests/test_layers_dense_gpu.py's rule
tol(T) = 8 . max(max|T_f32 - T_f64|, 2^-24 . max|T_f64|), which tests/test_transformer_reference.py shows to be 100 times finer than
any WRONG variant."""
import numpy as np
import pytest

import transformer_reference as T

pytestmark = pytest.mark.gpu

_REFERENCES = {}


def _dev(torch, a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


@pytest.fixture(scope="module")
def forms(qgtc):
    """[(label, adjacency, view)]: plain, transposed, reordered, reordered transposed"""
    import torch

    src, dst, _ = T.GRAPH
    s, d = _dev(torch, src), _dev(torch, dst)
    plain = qgtc.pack_edges_tiled(s, d, T.N_NODES)
    moved = qgtc.pack_edges_tiled(s, d, T.N_NODES, reorder=True)
    assert plain.perm is None and moved.perm is not None
    return [("adj", plain, "adj"), ("adj.T", plain.T, "adj.T"), ("reordered adj", moved, "adj"), ("reordered adj.T", moved.T, "adj.T")]


def _reference(case, view, dtype_name="float64"):
    """The dense definition, computed once per (case, view) and left unchanged."""
    import torch

    key = (case.name, view, dtype_name)
    if key not in _REFERENCES:
        _REFERENCES[key] = case.reference(view, getattr(torch, dtype_name))
    return _REFERENCES[key]


def _run(torch, case, a):
    from qgtc_ppopp22_amd.conv import TransformerConv

    t = case.inputs()
    layer = TransformerConv(T.F_IN, T.OUT, heads=case.heads, concat=case.concat).cuda()
    params = {"dW_q": layer.W_q, "dW_k": layer.W_k, "dW_v": layer.W_v}
    with torch.no_grad():
        for name, prm in params.items():
            assert prm.shape == t[name[1:]].shape
            prm.copy_(_dev(torch, t[name[1:]], torch.float32))
    X = _dev(torch, t["X"], torch.float32).requires_grad_(True)
    Y = layer(a, X)
    Y.backward(_dev(torch, t["dY"], torch.float32))
    out = {"Y": Y, "dX": X.grad}
    out.update({name: prm.grad for name, prm in params.items()})
    return {k: v.detach().cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("case", T.CASES, ids=repr)
def test_within_the_reference_tolerance(qgtc, forms, case):
    """Every tensor within tol(T); the message lists the largest |got - T_f64| / tol(T) of every tensor on every form."""
    import torch

    lines, worst = [], 0.0
    for label, a, view in forms:
        want = _reference(case, view)
        tol = T.tolerances(want, _reference(case, view, "float32"))
        got = _run(torch, case, a)
        assert set(got) == set(want)
        for name in sorted(want):
            w = want[name].numpy()
            assert got[name].dtype == np.float32 and got[name].shape == w.shape and tol[name] > 0
            err = np.abs(got[name].astype(np.float64) - w)
            ratio = float(err.max()) / tol[name] if np.isfinite(err).all() else float("inf")
            worst = max(worst, ratio)
            lines.append(f"ratio {case.name} | {label} | {name} | {ratio:.3f} | tol {tol[name]:.3e}")
    print("\n".join(lines))
    assert worst <= 1.0, "\n".join(lines)


def test_only_a_tiled_adjacency_is_taken(qgtc):
    import torch
    from qgtc_ppopp22_amd.conv import TransformerConv

    layer = TransformerConv(T.F_IN, T.OUT).cuda()
    with pytest.raises(NotImplementedError):
        layer(torch.zeros((T.N_NODES, T.N_NODES), device="cuda"), torch.zeros((T.N_NODES, T.F_IN), device="cuda"))
    with pytest.raises(ValueError):
        TransformerConv(T.F_IN, T.OUT, heads=0)
