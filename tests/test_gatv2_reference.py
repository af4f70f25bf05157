"""The dense definition of conv.GATv2Conv (tests/gatv2_reference.py) against itself: every case keeps its leaky-relu arguments 64 times
further from the kink than its own float32 error, its float32 evaluation lies within rounding of float64, its gradients are the
derivative of its forward (central differences in float64), and every WRONG variant lies far outside the tolerance the GPU test allows,
so the inputs of tests/test_gatv2_dense_gpu.py tell each mistake from the definition. No GPU."""
import numpy as np
import pytest
import torch

import gatv2_reference as G


@pytest.mark.parametrize("view", G.VIEWS)
@pytest.mark.parametrize("case", G.CASES, ids=repr)
def test_no_float32_order_can_flip_a_branch(case, view):
    least, err = case.margin(view)
    print(f"{case.name} {view}: min |u_f64| {least:.3e}, max |u_f32 - u_f64| {err:.3e}, ratio {least / err:.1f}")
    assert err > 0 and least >= G.KINK_MARGIN * err
    case.reference(view)   # and the reference asserts it itself


@pytest.mark.parametrize("view", G.VIEWS)
@pytest.mark.parametrize("case", G.CASES, ids=repr)
def test_float32_is_float64_up_to_rounding(case, view):
    ref64, ref32 = case.reference(view), case.reference(view, torch.float32)
    tol = G.tolerances(ref64, ref32)
    assert set(ref64) == {"Y", "dX", "dW_l", "datt"} | (set() if case.shared else {"dW_r"})
    for name, v in tol.items():
        assert ref32[name].dtype == torch.float32 and 0 < v < 1e-3 * float(ref64[name].abs().max()), (name, v)


@pytest.mark.parametrize("view", G.VIEWS)
@pytest.mark.parametrize("case", G.CASES, ids=repr)
def test_gradients_are_the_derivative(case, view):
    src, dst, _ = G.GRAPH
    t = case.inputs()
    ref = case.reference(view)
    rng = np.random.default_rng(3)
    h = 1e-7   # far below the case's smallest |u|: no step crosses the kink

    def forward(**moved):
        u = dict(t, **moved)
        if case.shared and "W_l" in moved:
            u["W_r"] = u["W_l"]
        Y = G.gatv2_layer(src, dst, G.N_NODES, u["X"], u["W_l"], u["W_r"], u["att"], t["dY"], view=view, heads=case.heads,
                          concat=case.concat, shared=case.shared)["Y"]
        return float((Y * torch.from_numpy(t["dY"])).sum())

    names = [("X", "dX"), ("W_l", "dW_l"), ("att", "datt")] + ([] if case.shared else [("W_r", "dW_r")])
    for name, grad in names:
        direction = rng.standard_normal(t[name].shape)
        num = (forward(**{name: t[name] + h * direction}) - forward(**{name: t[name] - h * direction})) / (2 * h)
        want = float((ref[grad] * torch.from_numpy(direction)).sum())
        assert abs(num - want) <= 1e-5 * max(1.0, abs(want)), (name, num, want)


def test_rows_without_neighbours_give_zero():
    src, dst, _ = G.GRAPH
    for view in G.VIEWS:
        m = G.R.dense_adjacency(src, dst, G.N_NODES, view)
        empty = ~m.any(axis=1)
        assert empty.any(), "the graph has a row without neighbours on either view"
        Y = G.CASES[0].reference(view)["Y"].numpy()
        assert (Y[empty] == 0).all() and (Y[~empty] != 0).any()


@pytest.mark.parametrize("view", G.VIEWS)
@pytest.mark.parametrize("case", G.CASES, ids=repr)
def test_wrong_variants_lie_far_outside_the_tolerance(case, view):
    ref64, ref32 = case.reference(view), case.reference(view, torch.float32)
    tol = G.tolerances(ref64, ref32)
    for wrong in G.WRONG:
        if case.shared and wrong == "ends_swapped":
            continue   # with one matrix both ends are transformed alike
        bad = case.reference(view, wrong=wrong)
        ratios = {k: float((bad[k] - ref64[k]).abs().max()) / tol[k] for k in ref64}
        print(f"{case.name} {view} {wrong}: " + ", ".join(f"{k} {r:.0f}" for k, r in ratios.items()))
        assert min(ratios.values()) > 100, (wrong, ratios)
