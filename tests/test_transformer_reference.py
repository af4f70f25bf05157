"""The dense definition of conv.TransformerConv (tests/transformer_reference.py) against itself: its gradients are the derivative of
its forward (central differences in float64), and every WRONG variant lies far outside the tolerance the GPU test allows, so the
inputs of tests/test_transformer_dense_gpu.py tell each mistake from the definition. No GPU."""
import numpy as np
import pytest
import torch

import transformer_reference as T


@pytest.mark.parametrize("view", T.VIEWS)
@pytest.mark.parametrize("case", T.CASES, ids=repr)
def test_gradients_are_the_derivative(case, view):
    src, dst, _ = T.GRAPH
    t = case.inputs()
    ref = case.reference(view)
    rng = np.random.default_rng(3)
    h = 1e-6

    def forward(**moved):
        u = dict(t, **moved)
        Y = T.transformer_layer(src, dst, T.N_NODES, u["X"], u["W_q"], u["W_k"], u["W_v"], t["dY"], view=view, heads=case.heads,
                                concat=case.concat)["Y"]
        return float((Y * torch.from_numpy(t["dY"])).sum())

    for name, grad in (("X", "dX"), ("W_q", "dW_q"), ("W_k", "dW_k"), ("W_v", "dW_v")):
        direction = rng.standard_normal(t[name].shape)
        num = (forward(**{name: t[name] + h * direction}) - forward(**{name: t[name] - h * direction})) / (2 * h)
        want = float((ref[grad] * torch.from_numpy(direction)).sum())
        assert abs(num - want) <= 1e-6 * max(1.0, abs(want)), (name, num, want)


def test_rows_without_neighbours_give_zero():
    src, dst, _ = T.GRAPH
    for view in T.VIEWS:
        m = T.R.dense_adjacency(src, dst, T.N_NODES, view)
        empty = ~m.any(axis=1)
        assert empty.any(), "the graph has a row without neighbours on either view"
        Y = T.CASES[0].reference(view)["Y"].numpy()
        assert (Y[empty] == 0).all() and (Y[~empty] != 0).any()


@pytest.mark.parametrize("view", T.VIEWS)
@pytest.mark.parametrize("case", T.CASES, ids=repr)
def test_wrong_variants_lie_far_outside_the_tolerance(case, view):
    ref64, ref32 = case.reference(view), case.reference(view, torch.float32)
    tol = T.tolerances(ref64, ref32)
    for name, v in tol.items():
        assert 0 < v < 1e-3 * float(ref64[name].abs().max()), (name, v)
    for wrong in T.WRONG:
        bad = case.reference(view, wrong=wrong)
        ratios = {k: float((bad[k] - ref64[k]).abs().max()) / tol[k] for k in ref64}
        print(f"{case.name} {view} {wrong}: " + ", ".join(f"{k} {r:.0f}" for k, r in ratios.items()))
        assert min(ratios[k] for k in ("Y", "dX", "dW_q", "dW_k", "dW_v")) > 100, (wrong, ratios)
