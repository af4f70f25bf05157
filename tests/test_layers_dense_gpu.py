"""conv.GCNConv, conv.GATConv and sage.SAGEConv (whole neighbourhoods, fixed-fanout samples, two layers over the blocks of a mini-batch)
on the device against the dense float64 definitions of tests/layers_reference.py, gradients included. Every case runs the real layer on ``adj``, on ``adj.T`` and on both views of ``pack_edges_tiled(..., reorder=True)`` of the
same edge list, with the parameters the reference used; X and the result are in the edge list's numbering and every element is
compared. On the dyadic graph with integer data all arithmetic is exact (tests/test_layers_reference.py proves it for these inputs), so
the four forms give the reference's bits; on the random graph every tensor lies within the tolerance the reference computes for it,
tol(T) = 8 . max(max|T_f32 - T_f64|, 2^-24 . max|T_f64|), which the same CPU test shows to be 100 times finer than any WRONG variant."""
import numpy as np
import pytest

import layers_reference as R
from layers_reference import CLASSES, DROP_RATE, DROP_SEED, EXACT_CASES, F_IN, GAT_OUT, HIDDEN, N_NODES, TOLERANCE_CASES

pytestmark = pytest.mark.gpu

_REFERENCES = {}


def _dev(torch, a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


@pytest.fixture(scope="module")
def forms(qgtc):
    """{graph: [(label, adjacency, view, rank)]}: plain, transposed, reordered, reordered transposed; rank (numpy, rank[old] = new) is
    None without reorder."""
    import torch

    out = {}
    for name, (src, dst, _) in R.GRAPHS.items():
        s, d = _dev(torch, src), _dev(torch, dst)
        plain = qgtc.pack_edges_tiled(s, d, N_NODES)
        moved = qgtc.pack_edges_tiled(s, d, N_NODES, reorder=True)
        assert plain.perm is None and moved.perm is not None
        rank = moved.rank.cpu().numpy()
        assert not np.array_equal(rank, np.arange(N_NODES)) and np.array_equal(np.sort(rank), np.arange(N_NODES))
        out[name] = [("adj", plain, "adj", None), ("adj.T", plain.T, "adj.T", None), ("reordered adj", moved, "adj", rank),
                     ("reordered adj.T", moved.T, "adj.T", rank)]
    return out


def _reference(case, view, rank, dtype_name="float64"):
    """The dense definition, computed once per (case, view, numbering it depends on) and left unchanged."""
    import torch

    rank = rank if case.uses_rank else None
    key = (case.name, view, None if rank is None else rank.tobytes(), dtype_name)
    if key not in _REFERENCES:
        _REFERENCES[key] = {k: v.numpy() for k, v in case.reference(view, getattr(torch, dtype_name), rank=rank).items()}
    return _REFERENCES[key]


def _run(torch, qgtc, case, a, train=True, dense=None):
    """{name: float32 numpy}: the real layer's output and gradients on the adjacency (view) ``a``, or on the dense matrix ``dense``."""
    from qgtc_ppopp22_amd.conv import GATConv, GCNConv
    from qgtc_ppopp22_amd.tiled import edge_slots, edge_values

    if case.kind == "sage":
        assert dense is None and train
        return _run_sage(torch, case, a)
    t, o = case.inputs(), case.options
    src, dst, nodes = case.graph()
    X = _dev(torch, t["X"], torch.float32).requires_grad_(True)
    kw = {}
    if o.get("nodes"):
        kw["nodes"] = _dev(torch, nodes)
    if o.get("drop"):
        kw["edge_seed"] = DROP_SEED
    rate = DROP_RATE if o.get("drop") else 0.0
    if case.kind == "gcn":
        layer = GCNConv(F_IN, HIDDEN, CLASSES, norm=o.get("norm"), aggr=o.get("aggr", "sum"), edge_drop=rate).cuda()
        params = {"dW_in": (layer.W_in, t["W_in"]), "dW_out": (layer.W_out, t["W_out"])}
    else:
        layer = GATConv(F_IN, GAT_OUT, heads=o["heads"], negative_slope=o["slope"], concat=o["concat"], edge_drop=rate).cuda()
        params = {"dW": (layer.W, t["W"]), "da_dst": (layer.a_dst, t["a_dst"]), "da_src": (layer.a_src, t["a_src"])}
    with torch.no_grad():
        for prm, value in params.values():
            assert prm.shape == value.shape
            prm.copy_(_dev(torch, value, torch.float32))
    layer.train(train)
    ew = None
    if "EW" in t:
        r, c = np.nonzero(R.cells(src, dst, N_NODES))                       # the stored cells, each once, in the edge list's numbering
        r_dev, c_dev = _dev(torch, r), _dev(torch, c)
        ew = edge_values(a, r_dev, c_dev, _dev(torch, t["EW"][r, c], torch.float32)).requires_grad_(True)
        kw["edge_weight"] = ew
    Y = layer(a if dense is None else dense, X, **kw)
    Y.backward(_dev(torch, t["dY"], torch.float32))
    out = {"Y": Y, "dX": X.grad}
    out.update({name: prm.grad for name, (prm, _) in params.items()})
    got = {k: v.detach().cpu().numpy() for k, v in out.items()}
    if ew is not None:
        slots = edge_slots(a, r_dev, c_dev).cpu().numpy()
        assert slots.min() >= 0 and np.unique(slots).size == slots.size == ew.numel()
        got["dEW"] = np.zeros((N_NODES, N_NODES), dtype=np.float32)
        got["dEW"][r, c] = ew.grad.cpu().numpy()[slots]
    for v in got.values():
        assert v.dtype == np.float32
    return got


def _run_sage(torch, case, a):
    """{name: float32 numpy}: the real sage.SAGEConv on the adjacency (view) ``a`` with the case's parameters - one layer, or two over
    fanout.sample_blocks of the view with the batch loss. X, dY and the batch flags are in the edge list's numbering, and so is every
    result; the seed flags are moved as a user must move them, ``node_bitmap(a.to_new(flags), n)``."""
    from qgtc_ppopp22_amd import fanout as fo
    from qgtc_ppopp22_amd.sage import SAGEConv
    from qgtc_ppopp22_amd.tiled import node_bitmap

    t, o = case.inputs(), case.options
    k = o.get("fanout")
    layers = []
    for l, (Ws, b, Wn) in enumerate(case.sage_params(t)):
        # a block's layer draws nothing, and a layer of the whole neighbourhood has no fanout or is in eval()
        layer = SAGEConv(Ws.shape[1], Ws.shape[0], aggr=o["aggr"], fanout=k if isinstance(k, int) else 4 if o.get("eval") else None).cuda()
        with torch.no_grad():
            for prm, value in ((layer.lin_self.weight, Ws), (layer.lin_self.bias, b), (layer.lin_nbr.weight, Wn)):
                assert prm.shape == value.shape
                prm.copy_(_dev(torch, value, torch.float32))
        layers.append(layer.train(not o.get("eval")))
    X = _dev(torch, t["X"], torch.float32).requires_grad_(True)
    dY = _dev(torch, t["dY"], torch.float32)
    if case.chained:
        flags = _dev(torch, R.batch_flags())
        blocks = fo.sample_blocks(a, node_bitmap(a.to_new(flags), N_NODES), k, DROP_SEED)
        h = X
        for layer, block in zip(layers, blocks):
            h = layer(a, h, block=block)
        (h * dY)[flags].sum().backward()
        out = {"Y": h[flags], "dX": X.grad}
        tags = ("0", "1")
    else:
        Y = layers[0](a, X, seed=DROP_SEED)
        Y.backward(dY)
        out = {"Y": Y, "dX": X.grad}
        tags = ("",)
    for tag, layer in zip(tags, layers):
        out.update({f"dW_self{tag}": layer.lin_self.weight.grad, f"db{tag}": layer.lin_self.bias.grad, f"dW_nbr{tag}": layer.lin_nbr.weight.grad})
    got = {name: v.detach().cpu().numpy() for name, v in out.items()}
    for v in got.values():
        assert v.dtype == np.float32
    return got


def _mismatches(got, want, label):
    """The tensors that are not the reference's bits after the cast (equal-valued -0 and +0 count as equal, and only there)."""
    assert set(got) == set(want), (label, sorted(got), sorted(want))
    bad = []
    for name in sorted(want):
        assert got[name].shape == want[name].shape, (label, name)
        diff = got[name].astype(np.float64) != want[name]
        if diff.any():
            at = tuple(int(i) for i in np.argwhere(diff)[0])
            bad.append(f"{label} {name}: {int(diff.sum())} of {diff.size} elements, first at {at}: {got[name][at]!r} != {want[name][at]!r}")
    return bad


@pytest.mark.parametrize("case", EXACT_CASES, ids=repr)
def test_exact_cases_bit_for_bit(qgtc, forms, case):
    import torch

    bad = []
    for label, a, view, rank in forms["dyadic"]:
        bad += _mismatches(_run(torch, qgtc, case, a), _reference(case, view, rank), label)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", ["gcn-None", "gcn-sym"])
def test_eval_mode_is_the_layer_without_edge_drop(qgtc, forms, name):
    import torch

    plain = next(c for c in EXACT_CASES if c.name == name)
    dropping = R.Case(plain.name, plain.kind, True, (), plain.denominator, drop=True, **plain.options)
    bad = []
    for label, a, view, rank in forms["dyadic"]:
        bad += _mismatches(_run(torch, qgtc, dropping, a, train=False), _reference(plain, view, rank), label)
    assert not bad, "\n".join(bad)


def test_dense_matrix_gives_the_same_bits(qgtc):
    """norm=None on the dense 0/1 matrix of either view: the torch.mm route of GCNConv.forward."""
    import torch

    case = next(c for c in EXACT_CASES if c.name == "gcn-None")
    src, dst, _ = case.graph()
    bad = []
    for view in R.VIEWS:
        A = _dev(torch, R.dense_adjacency(src, dst, N_NODES, view), torch.float32)
        bad += _mismatches(_run(torch, qgtc, case, None, dense=A), _reference(case, view, None), f"dense {view}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("case", TOLERANCE_CASES, ids=repr)
def test_tolerance_cases_within_the_reference_tolerance(qgtc, forms, case):
    """Every tensor within tol(T); the message lists the largest |got - T_f64| / tol(T) of every tensor on every form."""
    import torch

    lines, worst = [], 0.0
    for label, a, view, rank in forms["random"]:
        want = _reference(case, view, rank)
        tol = R.tolerances({k: torch.from_numpy(v) for k, v in want.items()},
                           {k: torch.from_numpy(v) for k, v in _reference(case, view, rank, "float32").items()})
        got = _run(torch, qgtc, case, a)
        assert set(got) == set(want)
        for name in sorted(want):
            assert got[name].shape == want[name].shape and tol[name] > 0
            err = np.abs(got[name].astype(np.float64) - want[name])
            ratio = float(err.max()) / tol[name] if np.isfinite(err).all() else float("inf")
            worst = max(worst, ratio)
            lines.append(f"ratio {case.name} | {label} | {name} | {ratio:.3f} | tol {tol[name]:.3e}")
    print("\n".join(lines))
    assert worst <= 1.0, "\n".join(lines)
