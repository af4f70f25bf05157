"""conv.GATv2Conv on the device against the dense float64 definition of tests/gatv2_reference.py, gradients for X, W_l, W_r and att
included. Every case runs the real layer on ``adj``, on ``adj.T`` and on both views of ``pack_edges_tiled(..., reorder=True)`` of the
same edge list, with the parameters the reference used; X and the result are in the edge list's numbering and every element is
compared. Every tensor lies within the tolerance the reference computes for it, tests/test_layers_dense_gpu.py's rule
tol(T) = 8 . max(max|T_f32 - T_f64|, 2^-24 . max|T_f64|); the reference asserts for every case that no float32 evaluation order can
flip a branch of the leaky relu, and tests/test_gatv2_reference.py shows the tolerance to be 100 times finer than any WRONG variant."""
import numpy as np
import pytest

import gatv2_reference as G

pytestmark = pytest.mark.gpu

_REFERENCES = {}


def _dev(torch, a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


@pytest.fixture(scope="module")
def forms(qgtc):
    """[(label, adjacency, view)]: plain, transposed, reordered, reordered transposed"""
    import torch

    src, dst, _ = G.GRAPH
    s, d = _dev(torch, src), _dev(torch, dst)
    plain = qgtc.pack_edges_tiled(s, d, G.N_NODES)
    moved = qgtc.pack_edges_tiled(s, d, G.N_NODES, reorder=True)
    assert plain.perm is None and moved.perm is not None
    return [("adj", plain, "adj"), ("adj.T", plain.T, "adj.T"), ("reordered adj", moved, "adj"), ("reordered adj.T", moved.T, "adj.T")]


def _reference(case, view, dtype_name="float64"):
    """The dense definition, computed once per (case, view) and left unchanged."""
    import torch

    key = (case.name, view, dtype_name)
    if key not in _REFERENCES:
        _REFERENCES[key] = case.reference(view, getattr(torch, dtype_name))
    return _REFERENCES[key]


def _layer(torch, case):
    from qgtc_ppopp22_amd.conv import GATv2Conv

    t = case.inputs()
    layer = GATv2Conv(G.F_IN, G.OUT, heads=case.heads, negative_slope=G.SLOPE, concat=case.concat, share_weights=case.shared).cuda()
    params = {"dW_l": layer.W_l, "datt": layer.att}
    if not case.shared:
        params["dW_r"] = layer.W_r
    with torch.no_grad():
        for name, prm in params.items():
            assert prm.shape == t[name[1:]].shape
            prm.copy_(_dev(torch, t[name[1:]], torch.float32))
    return layer, params, t


def _run(torch, case, a):
    layer, params, t = _layer(torch, case)
    X = _dev(torch, t["X"], torch.float32).requires_grad_(True)
    Y = layer(a, X)
    Y.backward(_dev(torch, t["dY"], torch.float32))
    out = {"Y": Y, "dX": X.grad}
    out.update({name: prm.grad for name, prm in params.items()})
    return {k: v.detach().cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("case", G.CASES, ids=repr)
def test_within_the_reference_tolerance(qgtc, forms, case):
    """Every tensor within tol(T); the message lists the largest |got - T_f64| / tol(T) of every tensor on every form."""
    import torch

    lines, worst = [], 0.0
    for label, a, view in forms:
        want = _reference(case, view)
        tol = G.tolerances(want, _reference(case, view, "float32"))
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


def test_shared_weights_tie_the_gradients(qgtc, forms):
    """share_weights=True: W_r IS W_l, one parameter, and its gradient is the sum of what the two matrices of an untied layer with the
    same values receive (the tied case of test_within_the_reference_tolerance holds the sum against the definition)."""
    import torch
    from qgtc_ppopp22_amd.conv import GATv2Conv

    case = next(c for c in G.CASES if c.shared)
    layer, params, t = _layer(torch, case)
    assert layer.W_r is layer.W_l and len(list(layer.parameters())) == 2
    free = GATv2Conv(G.F_IN, G.OUT, heads=case.heads, negative_slope=G.SLOPE, concat=case.concat).cuda()
    assert free.W_r is not free.W_l and len(list(free.parameters())) == 3
    with torch.no_grad():
        free.W_l.copy_(layer.W_l)
        free.W_r.copy_(layer.W_l)
        free.att.copy_(layer.att)
    _, a, view = forms[2]
    X, dY = _dev(torch, t["X"], torch.float32), _dev(torch, t["dY"], torch.float32)
    Y = layer(a, X)
    Y.backward(dY)
    Y2 = free(a, X)
    Y2.backward(dY)
    assert torch.equal(Y.view(torch.int32), Y2.view(torch.int32)), "the same values, the same forward bits"
    tied, summed = layer.W_l.grad, free.W_l.grad + free.W_r.grad
    tol = G.tolerances(_reference(case, view), _reference(case, view, "float32"))["dW_l"]
    assert float((tied - summed).abs().max()) <= tol
    assert torch.equal(layer.att.grad.view(torch.int32), free.att.grad.view(torch.int32))


@pytest.mark.parametrize("train", [False, True])
def test_two_runs_give_the_same_bits(qgtc, forms, train):
    import torch

    case = G.CASES[1]
    layer, params, t = _layer(torch, case)
    layer.train(train)
    X, dY = _dev(torch, t["X"], torch.float32), _dev(torch, t["dY"], torch.float32)
    for _, a, _ in forms:
        runs = []
        for _ in range(2):
            layer.zero_grad()
            Xg = X.clone().requires_grad_(True)
            Y = layer(a, Xg)
            Y.backward(dY)
            runs.append([Y.detach(), Xg.grad] + [p.grad.clone() for p in layer.parameters()])
        for x, y in zip(*runs):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_the_layer_trains_on_a_reordered_adjacency(qgtc):
    """INTEGRATION.md's snippet: a few Adam steps on a reordered adjacency with self loops lower the loss at every step."""
    import torch
    from qgtc_ppopp22_amd.conv import GATv2Conv

    src, dst, _ = G.GRAPH
    s, d = qgtc.add_self_loops(_dev(torch, src), _dev(torch, dst), G.N_NODES)
    adj = qgtc.pack_edges_tiled(s, d, G.N_NODES, reorder=True)
    torch.manual_seed(0)
    rng = np.random.default_rng(11)
    labels = _dev(torch, rng.integers(0, 8, size=G.N_NODES))
    X = _dev(torch, rng.standard_normal((G.N_NODES, G.F_IN)), torch.float32) + torch.nn.functional.one_hot(labels, G.F_IN).float()
    layer = GATv2Conv(G.F_IN, 8, heads=8, concat=False).cuda()
    opt = torch.optim.Adam(layer.parameters(), lr=0.01)
    losses = []
    for _ in range(5):
        opt.zero_grad()
        loss = torch.nn.functional.cross_entropy(layer(adj.T, X), labels)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    print("losses", losses)
    assert all(b < a for a, b in zip(losses, losses[1:])), losses


def test_only_a_tiled_adjacency_is_taken(qgtc):
    import torch
    from qgtc_ppopp22_amd.conv import GATv2Conv

    layer = GATv2Conv(G.F_IN, G.OUT).cuda()
    with pytest.raises(NotImplementedError):
        layer(torch.zeros((G.N_NODES, G.N_NODES), device="cuda"), torch.zeros((G.N_NODES, G.F_IN), device="cuda"))
    with pytest.raises(ValueError):
        GATv2Conv(G.F_IN, G.OUT, heads=0)
    with pytest.raises(ValueError):
        GATv2Conv(G.F_IN, G.OUT, negative_slope=1.5)
