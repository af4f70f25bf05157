"""The dense layer definitions of tests/layers_reference.py checked on the CPU, on the very inputs tests/test_layers_dense_gpu.py
hands the real layers: the hand-written gradients are the derivatives of the forward, the dyadic cases are exact in float32 (with the
guard that makes them so), and every WRONG variant is told from the definition - by an element in the exact cases, by 100 times the
tolerance in the others. For the SAGE cases also what their samples rest on: kept degrees that are powers of two, nodes with more
neighbours than the fanout, a kept set that changes with the numbering, chains with a real frontier. No GPU, no call into the library."""
import numpy as np
import pytest
import torch

import layers_reference as R
import tiled_blocks_model as bm
import tiled_fanout_model as fm
from layers_reference import CASES, EXACT_CASES, N_NODES, TOLERANCE_CASES, VIEWS, WRONG

# a numbering other than the edge list's, for the cases whose reference depends on it (the GPU test takes the adjacency's own)
RANK = np.random.default_rng(5).permutation(N_NODES)
DEGREES = {0, 1, 4, 16}
SEPARATION = 100.0
NEED_A_NUMBERING = ("mask_in_old_numbering", "rows_not_moved", "batch_in_old_numbering")   # they show under a non-identity rank only


def _ranks(case):
    return (None, RANK) if case.uses_rank else (None,)


# ---- the graphs ---------------------------------------------------------------------------------------------------------------------

def test_dyadic_graph_is_as_stated():
    src, dst, nodes = R.dyadic_graph(2024)
    n = N_NODES
    a = R.cells(src, dst, n)
    out_deg, in_deg = a.sum(axis=1), a.sum(axis=0)
    assert set(out_deg.tolist()) == DEGREES and set(in_deg.tolist()) == DEGREES
    assert int((out_deg != in_deg).sum()) >= 16
    count = np.zeros((n, n), dtype=np.int64)
    np.add.at(count, (src, dst), 1)
    assert int((count == 3).sum()) == 50 and int((count == 2).sum()) == 40 and count.max() == 3
    assert int(a.sum()) == 16 * 16 + 16 * 4 + 4 + 64 * 4 + 128 * 16 + 40
    # the cells scatter over every row block and k-quad, the partial last ones included
    r, c = np.nonzero(a)
    assert set((r // 32).tolist()) == set(range(10)) and set((c // 128).tolist()) == set(range(3))
    # the induced subgraph keeps the degree set, and differs from the whole graph's degrees on its nodes
    sub = a & nodes[:, None] & nodes[None, :]
    assert set(sub.sum(axis=1).tolist()) <= DEGREES and set(sub.sum(axis=0).tolist()) <= DEGREES
    assert int((sub.sum(axis=1)[nodes] != out_deg[nodes]).sum()) >= 4 and int((sub.sum(axis=0)[nodes] != in_deg[nodes]).sum()) >= 4
    assert int(((count == 2) & nodes[:, None] & nodes[None, :]).sum()) >= 20
    assert np.array_equal(R.dense_adjacency(src, dst, n, "adj.T"), a.T) and not np.array_equal(a, a.T)


def test_random_graph_is_directed_with_doubled_edges():
    src, dst, nodes = R.random_graph(2025)
    n = N_NODES
    a = R.cells(src, dst, n)
    count = np.zeros((n, n), dtype=np.int64)
    np.add.at(count, (src, dst), 1)
    assert int((count == 2).sum()) > 0 and int((count >= 3).sum()) > 0 and 5 * n < src.size < 9 * n
    assert int((a != a.T).sum()) > n and int((a.sum(axis=1) != a.sum(axis=0)).sum()) > n // 2
    assert 100 < int(nodes.sum()) < 200


def test_the_multiplicity_rule():
    src, dst = np.array([0, 1, 1, 2, 2, 2, 3, 3, 3, 3]), np.array([1, 2, 2, 0, 0, 0, 3, 3, 3, 3])
    want = np.zeros((4, 4), dtype=bool)
    want[0, 1] = want[2, 0] = want[3, 3] = True
    assert np.array_equal(R.cells(src, dst, 4), want)
    assert R.cells(src, dst, 4, "multiplicity_kept")[1, 2]


# ---- the gradients are the forward's derivatives ------------------------------------------------------------------------------------

def _directional(run, tensors, grads, dY, eps):
    """For every parameter: <grad, D> against the central difference of <Y, dY> along a random direction D."""
    rng = np.random.default_rng(1)
    for name, grad_name in grads.items():
        D = rng.standard_normal(tensors[name].shape)
        if name == "EW":
            D = D * (tensors[name] != 0)
        up, down = dict(tensors), dict(tensors)
        up[name], down[name] = tensors[name] + eps * D, tensors[name] - eps * D
        numeric = (float((run(up)["Y"] * torch.as_tensor(dY)).sum()) - float((run(down)["Y"] * torch.as_tensor(dY)).sum())) / (2 * eps)
        analytic = float((run(tensors)[grad_name] * torch.as_tensor(D)).sum())
        assert abs(numeric - analytic) <= 1e-6 * max(1.0, abs(analytic)), (name, numeric, analytic)


@pytest.mark.parametrize("view", VIEWS)
@pytest.mark.parametrize("options", [dict(norm=None), dict(norm="mean"), dict(norm="sym", nodes=True), dict(norm="sym", drop=True),
                                     dict(edge_weight=True), dict(aggr="max"), dict(aggr="min", drop=True)], ids=str)
def test_gcn_gradients_are_the_derivatives(options, view):
    src, dst, nodes = R.random_graph(7)
    n, rng = N_NODES, np.random.default_rng(3)
    t = {"X": rng.standard_normal((n, 5)), "W_in": rng.standard_normal((5, 6)), "W_out": rng.standard_normal((6, 3))}
    dY = rng.standard_normal((n, 3))
    grads = {"X": "dX", "W_in": "dW_in", "W_out": "dW_out"}
    if options.get("edge_weight"):
        t["EW"] = (rng.standard_normal((n, n)) + 3.0) * R.cells(src, dst, n)
        grads["EW"] = "dEW"

    def run(v):
        return R.gcn_layer(src, dst, n, v["X"], v["W_in"], v["W_out"], dY, view=view, norm=options.get("norm"),
                           aggr=options.get("aggr", "sum"), nodes=nodes if options.get("nodes") else None, edge_weight=v.get("EW"),
                           edge_drop=(0.5, 11, RANK) if options.get("drop") else None, rank=RANK)

    _directional(run, t, grads, dY, 1e-6)


@pytest.mark.parametrize("view", VIEWS)
@pytest.mark.parametrize("options", [dict(heads=1, concat=True), dict(heads=3, concat=True, nodes=True), dict(heads=3, concat=False, drop=True)],
                         ids=str)
def test_gat_gradients_are_the_derivatives(options, view):
    src, dst, nodes = R.random_graph(7)
    n, rng, heads = N_NODES, np.random.default_rng(4), options["heads"]
    t = {"X": rng.standard_normal((n, 5)), "W": rng.standard_normal((5, heads * 4)) / 2, "a_dst": rng.standard_normal((heads, 4)) / 2,
         "a_src": rng.standard_normal((heads, 4)) / 2}
    dY = rng.standard_normal((n, heads * 4 if options["concat"] else 4))

    def run(v):
        return R.gat_layer(src, dst, n, v["X"], v["W"], v["a_dst"], v["a_src"], dY, view=view, heads=heads, concat=options["concat"],
                           negative_slope=0.1, nodes=nodes if options.get("nodes") else None,
                           edge_drop=(0.5, 11, RANK) if options.get("drop") else None)

    _directional(run, t, {"X": "dX", "W": "dW", "a_dst": "da_dst", "a_src": "da_src"}, dY, 1e-6)


@pytest.mark.parametrize("view", VIEWS)
@pytest.mark.parametrize("options", [dict(aggr="mean"), dict(aggr="max"), dict(aggr="mean", fanout=3), dict(aggr="max", fanout=3),
                                     dict(aggr="mean", fanout=(3, 2)), dict(aggr="max", fanout=(3, 2))], ids=str)
def test_sage_gradients_are_the_derivatives(options, view):
    """torch.autograd's gradients of the dense SAGE definition against central differences, for one layer and for the chain with the
    batch loss; standard-normal data, so no maximum is tied."""
    src, dst, _ = R.random_graph(7)
    n, rng = N_NODES, np.random.default_rng(6)
    chained = isinstance(options.get("fanout"), tuple)
    dims = (5, 6, 3) if chained else (5, 6)
    t = {"X": rng.standard_normal((n, dims[0]))}
    grads = {"X": "dX"}
    for l, (fi, fo) in enumerate(zip(dims, dims[1:])):
        tag = str(l) if chained else ""
        t[f"W_self{l}"], t[f"b{l}"], t[f"W_nbr{l}"] = rng.standard_normal((fo, fi)), rng.standard_normal(fo), rng.standard_normal((fo, fi))
        grads.update({f"W_self{l}": f"dW_self{tag}", f"b{l}": f"db{tag}", f"W_nbr{l}": f"dW_nbr{tag}"})
    dY = rng.standard_normal((n, dims[-1]))
    batch = R.batch_flags() if chained else None

    def run(v):
        params = [(v[f"W_self{l}"], v[f"b{l}"], v[f"W_nbr{l}"]) for l in range(len(dims) - 1)]
        return R.sage_layer(src, dst, n, v["X"], params, dY, view=view, aggr=options["aggr"], fanout=options.get("fanout"), batch=batch,
                            seed=11, rank=RANK)

    assert run(t)["Y"].shape == ((int(batch.sum()) if chained else n), dims[-1])
    _directional(run, t, grads, dY[batch] if chained else dY, 1e-6)      # a chain's Y holds the batch rows only


def _kept_degrees(src, dst, ids, k, axis, seed=R.DROP_SEED):
    """(kept cells as a set of (s, d) in the edge list's numbering, the kept degrees of the axis) of the fanout-k sample taken on ids"""
    s, d = np.nonzero(R.cells(src, dst, N_NODES))
    ks, kd = fm.kept_edges(ids[s], ids[d], N_NODES, k, seed, axis)
    inv = np.argsort(ids)
    return set(zip(inv[ks].tolist(), inv[kd].tolist())), np.bincount(ks if axis == "row" else kd, minlength=N_NODES)


@pytest.mark.parametrize("axis", fm.AXES)
def test_sage_samples_are_dyadic_and_depend_on_the_numbering(axis):
    """What the exact sampled cases rest on: under k = 4 and k = 2 every kept degree of the dyadic graph is 0, 1, 2 or 4, some node has
    more than k neighbours (on the random graph under k = 3 too), and a sample taken in another numbering keeps other cells."""
    own = np.arange(N_NODES)
    for graph, k, degrees in (("dyadic", 4, {0, 1, 4}), ("dyadic", 2, {0, 1, 2}), ("random", 3, None)):
        src, dst, _ = R.GRAPHS[graph]
        a = R.cells(src, dst, N_NODES)
        deg = a.sum(axis=1 if axis == "row" else 0)
        assert int((deg > k).sum()) >= 50, "the sample drops something"
        here, kept_deg = _kept_degrees(src, dst, own, k, axis)
        there, moved_deg = _kept_degrees(src, dst, RANK, k, axis)
        assert np.array_equal(kept_deg, np.minimum(deg, k)) and np.array_equal(np.sort(moved_deg), np.sort(kept_deg))
        assert degrees is None or set(kept_deg.tolist()) == degrees
        assert len(here) == len(there) == int(np.minimum(deg, k).sum()) < int(a.sum())
        print(f"{graph} k={k} {axis}: {len(here)} of {int(a.sum())} cells kept, {len(here ^ there)} differ under the relabelling")
        assert len(here ^ there) > (600 if graph == "dyadic" else len(here) // 4)


@pytest.mark.parametrize("axis", fm.AXES)
@pytest.mark.parametrize("graph, fanouts", [("dyadic", (4, 2)), ("random", (3, 2))])
def test_sage_chains_have_a_real_frontier(graph, fanouts, axis):
    """The chained cases: the batch is BATCH nodes, the last block's rows are the batch and the first block has rows outside it and
    inputs beyond its rows; on the dyadic graph the kept counts are {0, 1, 4} then {0, 1, 2}, in either numbering."""
    src, dst, _ = R.GRAPHS[graph]
    batch = R.batch_flags()
    assert int(batch.sum()) == R.BATCH == 24
    s, d = np.nonzero(R.cells(src, dst, N_NODES))
    kept = {}
    for name, ids in (("own", np.arange(N_NODES)), ("other", RANK)):
        moved = np.zeros(N_NODES, dtype=bool)
        moved[ids] = batch
        first, last = bm.blocks(ids[s], ids[d], N_NODES, axis, moved, fanouts, R.DROP_SEED)
        assert np.array_equal(last["rows"], moved) and np.array_equal(first["rows"], last["inputs"])
        rows, inputs = int(first["rows"].sum()), int(first["inputs"].sum())
        print(f"{graph} {fanouts} {axis} {name} numbering: {rows} rows and {inputs} inputs in the first block")
        assert R.BATCH < rows < inputs < N_NODES
        assert int((first["kept"] > 0).sum()) > R.BATCH and int((last["kept"] > 0).sum()) > 0
        if graph == "dyadic":
            assert set(first["kept"].tolist()) == {0, 1, 4} and set(last["kept"].tolist()) == {0, 1, 2}
        inv = np.argsort(ids)
        kept[name] = [set(zip(*(inv[e].tolist() for e in bm.kept_edges(ids[s], ids[d], N_NODES, b["k"], b["seed"], axis, b["rows"]))))
                      for b in (first, last)]
    assert kept["own"][0] != kept["other"][0] and kept["own"][1] != kept["other"][1]


def test_sage_cases_are_as_the_gpu_test_needs_them():
    sage = [c for c in CASES if c.kind == "sage"]
    assert [c.name for c in sage] == ["sage-mean", "sage-max", "sage-mean-fanout", "sage-max-fanout", "sage-mean-blocks", "sage-max-blocks",
                                      "sage-mean-random", "sage-mean-fanout-random", "sage-mean-blocks-random", "sage-max-blocks-random"]
    for c in sage:
        sampled = c.options.get("fanout") is not None
        assert c.uses_rank == (sampled or c.options["aggr"] == "max")
        assert ("rows_not_moved" in c.wrong) == c.uses_rank and ("mask_in_old_numbering" in c.wrong) == sampled
        assert ("batch_in_old_numbering" in c.wrong) == c.chained and ("mean_by_full_degree" in c.wrong) == (sampled and c.options["aggr"] == "mean")
        assert c.exact == (not c.name.endswith("-random")) and {"transposed", "multiplicity_kept"} <= set(c.wrong)
    assert {c.name: c.denominator for c in sage if c.exact} == {"sage-mean": 16, "sage-max": 1, "sage-mean-fanout": 4, "sage-max-fanout": 1,
                                                                "sage-mean-blocks": 8, "sage-max-blocks": 1}
    assert {c.name: c.options["fanout"] for c in sage if c.options.get("fanout")} == {
        "sage-mean-fanout": 4, "sage-max-fanout": 4, "sage-mean-blocks": (4, 2), "sage-max-blocks": (4, 2), "sage-mean-fanout-random": 3,
        "sage-mean-blocks-random": (3, 2), "sage-max-blocks-random": (3, 2)}


def test_leaky_relu_has_the_slope_at_zero():
    """With all scores 0 every logit is exactly 0: the gradient for a_src is the slope times what the identity would give."""
    case = next(c for c in EXACT_CASES if c.name == "gat-zero-h2-concat")
    src, dst, _ = case.graph()
    t = case.inputs()
    got = {s: R.gat_layer(src, dst, N_NODES, t["X"], t["W"], t["a_dst"], t["a_src"], t["dY"], heads=2, negative_slope=s)["da_src"]
           for s in (0.5, 1.0)}
    assert got[1.0].abs().max() > 0 and torch.equal(got[0.5], 0.5 * got[1.0])


# ---- the dyadic cases are exact -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("view", VIEWS)
@pytest.mark.parametrize("case", EXACT_CASES, ids=repr)
def test_exact_cases_are_exact_in_float32(case, view):
    largest = 0.0
    for rank in _ranks(case):
        rec = R.Record()
        ref64 = case.reference(view, torch.float64, rank=rank, record=rec)
        ref32 = case.reference(view, torch.float32, rank=rank)
        assert set(ref64) == set(ref32) and len(ref64) >= 4
        for name in ref64:
            assert ref32[name].dtype == torch.float32 and ref64[name].dtype == torch.float64
            assert torch.equal(ref32[name].to(torch.float64), ref64[name]), (name, rank is not None)
            assert ref64[name].abs().max() > 0 or name == "da_dst", name     # all logits equal: the row's softmax does not move with p
        # the guard: every intermediate is a multiple of 1 / denominator, and every partial sum behind it, in any order, is below 2^24
        # of those units, so float32 holds each of them exactly
        assert len(rec.items) >= 8
        if case.kind == "sage":     # autograd's gradients are the ones the record walked by hand, so its bounds cover them
            walked = {name: value for name, value, _ in rec.items if name in ref64}
            assert set(walked) == set(ref64) - {"Y"}
            for name, value in walked.items():
                assert torch.equal(value, ref64[name]), name
        for name, value, bound in rec.items:
            scaled = value * case.denominator
            assert torch.equal(scaled, scaled.round()), (name, "not a multiple of 1 /", case.denominator)
            assert float(bound.max()) * case.denominator < 2.0 ** 24, (name, float(bound.max()), case.denominator)
            largest = max(largest, float(bound.max()) * case.denominator)
    print(f"{case.name} {view}: largest bound {largest:.0f} of {2 ** 24}")


# ---- the inputs resolve the mistakes ------------------------------------------------------------------------------------------------

def separations(case, view, rank):
    """{variant: separation}: in an exact case the number of differing elements, otherwise the largest |wrong - right| / tol."""
    right = case.reference(view, torch.float64, rank=rank)
    tol = None if case.exact else R.tolerances(right, case.reference(view, torch.float32, rank=rank))
    out = {}
    for wrong in case.wrong:
        if wrong in NEED_A_NUMBERING and rank is None:
            continue
        got = case.reference(view, torch.float64, rank=rank, wrong=wrong)
        if case.exact:
            out[wrong] = float(sum(int((got[k] != right[k]).sum()) for k in right))
        else:
            out[wrong] = max(float((got[k] - right[k]).abs().max()) / tol[k] for k in right)
    return out


@pytest.mark.parametrize("view", VIEWS)
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_wrong_variants_differ(case, view):
    seen = set()
    for rank in _ranks(case):
        for wrong, sep in separations(case, view, rank).items():
            seen.add(wrong)
            print(f"separation {case.name} | {view} | {'other numbering' if rank is not None else 'own numbering'} | {wrong} | {sep:.4g}")
            assert sep >= (1 if case.exact else SEPARATION), (wrong, sep)
    assert seen == set(case.wrong)
    if not case.exact:
        ref64, ref32 = case.reference(view, torch.float64), case.reference(view, torch.float32)
        for name, tol in R.tolerances(ref64, ref32).items():
            err = float((ref32[name].to(torch.float64) - ref64[name]).abs().max())
            print(f"float32 {case.name} | {view} | {name} | {err:.3e} | {float(ref64[name].abs().max()):.3e} | {tol:.3e}")


def test_every_variant_applies_somewhere():
    for kind in (EXACT_CASES, TOLERANCE_CASES):
        assert {w for c in kind for w in c.wrong} >= set(WRONG) - ({"scores_swapped"} if kind is EXACT_CASES else
                                                                   {"full_graph_degrees", "no_keep_scale", "weights_transposed"})
    assert {w for c in CASES for w in c.wrong} == set(WRONG)


def test_tolerance_is_the_stated_formula():
    a64, a32 = {"T": torch.tensor([1.0, -4.0], dtype=torch.float64)}, {"T": torch.tensor([1.0, -4.0], dtype=torch.float32)}
    assert R.tolerances(a64, a32)["T"] == 8 * 2.0 ** -24 * 4.0       # the floor: a lucky exact float32 run
    a32["T"] = torch.tensor([1.0, -4.5], dtype=torch.float32)
    assert R.tolerances(a64, a32)["T"] == 8 * 0.5
