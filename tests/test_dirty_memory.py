"""The tables of tests/test_dirty_memory_gpu.py are complete, and its graphs and models are what the cases rely on. No GPU: the GPU
module imports without a device, and the models behind the directed cases are evaluated here on the graphs without an edge.

- every asynchronous entry of tests/stream_contract.py, and every entry a case of tests/stream_cases.py names outside the raw ``C.`` class,
  has a case that runs dirty; what is left out is exactly the two rules of the registry;
- every name of ``tiled.__all__`` and every ``torch.nn.Module`` of conv.py appears in the directed cases' tables: a new operator has to
  add its dirty-memory case;
- the graphs have the skips they are named for;
- the exact models take a graph without an edge and give what the float64 definitions give there (+0 everywhere, arg -1, nothing per
  edge), and the masks and the dropout seed of the ``masks`` case do what its docstring says."""
import types

import numpy as np
import pytest

import dirty_memory as dm
import stream_cases as sc
import test_dirty_memory_gpu as D
from stream_contract import ASYNC, CONTRACT, names_of


def test_every_entry_outside_the_raw_class_runs_dirty():
    dirty_entries = {e for c in D.REGISTRY for e in c.entries}
    for name in names_of(ASYNC):
        assert name in dirty_entries, f"{name} is asynchronous by tests/stream_contract.py and no case of it runs on dirty memory"
    named = {e for c in sc.CASES for e in c.entries if not e.startswith("C.")}
    assert named <= set(CONTRACT)
    assert not named - dirty_entries, f"entries whose cases are all left out: {sorted(named - dirty_entries)}"
    assert all(not c.raw for c in D.REGISTRY) and len({c.id for c in D.REGISTRY}) == len(D.REGISTRY)


def test_what_is_left_out_is_exactly_the_rule():
    """Raw cases (they prefill their own outputs), and the enqueue-graph cases on ENQUEUE_BIG shapes (run time); nothing else."""
    big = {f"enqueue-graph-{M}x{K}x{N}-w{w}-reps{r}-{lay}" for M, K, N, _, w, _ in sc.ENQUEUE_BIG for r in (1, 3, 200) for lay in ("rows", "cols")}
    raw = {c.id for c in sc.CASES if c.raw}
    assert big <= {c.id for c in sc.CASES} and len(big) == 24 and raw
    assert set(D.EXCLUDED) == big | raw
    assert {c.id for c in D.REGISTRY} == {c.id for c in sc.CASES} - big - raw
    assert all(c.entries == ("QGTC.bitMM2Bit_enqueue",) for c in sc.CASES if c.id in big)
    assert any(c.id.startswith("enqueue-graph-") for c in D.REGISTRY), "the small enqueue-graph shapes run dirty"
    # the plan objects allocate in their constructors and in bind(): every case of theirs is also BUILT on dirty memory
    planned = {c.id for c in D.REGISTRY if any(e.startswith(("QGTC.BatchedGemm.", "QGTC.FusedLayer.", "QGTC.ChainedPair.", "QGTC.EpochPlan.")) for e in c.entries)}
    assert planned == {c.id for c in D.BUILT_DIRTY} and len(planned) >= 10
    assert {e for c in D.BUILT_DIRTY for e in c.entries} >= {"QGTC.BatchedGemm.run", "QGTC.FusedLayer.run", "QGTC.ChainedPair.run", "QGTC.EpochPlan.run",
                                                             "QGTC.EpochPlan.run_launch", "QGTC.EpochPlan.bind"}


def test_every_operator_and_every_layer_has_a_directed_case():
    import torch

    from qgtc_ppopp22_amd import conv, tiled

    covered = {name for _, names in D.DIRECTED.values() for name in names}
    missing = sorted(set(tiled.__all__) - covered)
    assert not missing, f"tiled.__all__ names without a dirty-memory case in test_dirty_memory_gpu.DIRECTED: {missing}"
    assert covered <= set(tiled.__all__), sorted(covered - set(tiled.__all__))
    layers = {k for k, v in vars(conv).items() if isinstance(v, type) and issubclass(v, torch.nn.Module) and v.__module__ == conv.__name__}
    stepped = {cls for _, cls in D.MODULES.values()} | {"GCNConv_Qnt"}
    assert layers == stepped, f"layers of conv.py without a dirty-memory step: {sorted(layers - stepped)}; stale: {sorted(stepped - layers)}"
    assert D.QNT_MODES.keys() == {"sum", "mean", "float_out"}
    assert set(D.GRAPHS) == {"void1", "void129", "islands200", "g300", "g300r"}


def test_the_patterns_are_what_the_suite_already_uses():
    from test_tiled_variants_gpu import NAN_WORD, POISON_BITS

    assert dm.NAN_WORD == NAN_WORD == sc.NAN_WORD and dm.signed(dm.SMALL_WORD) == POISON_BITS
    f = np.array([dm.NAN_WORD, dm.SMALL_WORD], dtype=np.uint32).view(np.float32)
    assert np.isnan(f[0]) and -3e-16 < f[1] < -2.8e-16
    assert D.bit_shapes() == [(16, 3, 5), (24, 2, 8)]


def test_the_graphs_have_the_skips_they_are_named_for():
    from tiled_model import np_colindex, np_tiled

    for name, n, blocks in (("void1", 1, 1), ("void129", 129, 5)):
        g = D.graph(name)
        rp, kq, tiles = np_tiled(g.s, g.d, g.n)
        assert g.n == n and rp.size == blocks + 1 and not rp.any() and kq.size == 0 and tiles.shape == (0, 32, 4)
    assert (129 + 7) // 8 * 8 == 136 and (129 + 127) // 128 == 2            # PAD8 rows and a ragged second k-quad
    g = D.graph("islands200")
    rp, kq, _ = np_tiled(g.s, g.d, g.n)
    per_block = np.diff(rp)
    assert per_block.tolist() == [1, 0, 0, 0, 0, 0, 1], "row blocks 1 .. 5 without a tile between two that have one"
    assert g.n - 6 * 32 == 8 and kq.tolist() == [0, 1], "a last block with 8 live rows; k-quad 1 reached from that block only"
    col_ptr, _, col_rb = np_colindex(rp, kq, g.n)
    assert np.diff(col_ptr).tolist() == [1, 1] and col_rb.tolist() == [0, 6]
    in_deg = np.bincount(g.d, minlength=g.n)
    assert (in_deg == 0).sum() > 170, "most columns have no in-edge"
    for name in ("g300", "g300r"):
        g = D.graph(name)
        out_deg, in_deg = np.bincount(g.src, minlength=300), np.bincount(g.dst, minlength=300)
        assert in_deg[7] >= 299 and out_deg[5] == 0 and in_deg[9] == 0, "a hub column, a row and a column without edges"
        assert g.reorder == (name == "g300r") and (g.rank is not None) == g.reorder
    r = D.graph("g300r")
    assert sorted(r.rank.tolist()) == list(range(300)) and not np.array_equal(r.rank, np.arange(300))


@pytest.fixture(scope="module")
def cpu_env(oracle):
    """The operands of a case on the CPU: prepare() builds them and evaluates every model; run() is never called."""
    import torch

    return types.SimpleNamespace(torch=torch, dev=torch.device("cpu"), Q=None, tiled=None, O=oracle)


@pytest.mark.parametrize("name", ("void1", "void129"))
@pytest.mark.parametrize("case", sorted(D.DIRECTED))
def test_the_models_take_a_graph_without_an_edge(cpu_env, case, name):
    """Every model behind the directed cases accepts an empty edge list: prepare() evaluates all of them."""
    g = D.graph(name)
    inputs, run, want = D.DIRECTED[case][0](cpu_env, g)
    assert callable(run) and inputs and len(want) >= 10
    assert all(w is None or np.asarray(w).dtype.kind != "f" or np.isfinite(w).all() for w in want)


@pytest.mark.parametrize("n", (1, 129))
@pytest.mark.parametrize("transposed", (False, True))
def test_without_an_edge_the_models_give_the_float64_definition(n, transposed):
    """The float64 definitions on a graph without an edge: every sum is empty (+0), a maximum over nothing is +0 with winner -1, a
    softmax over nothing has inv = 0 and gives +0, its shift m is L(att_out + 0); there is no stored cell, so every per-edge vector is
    empty and every fold over an owner's cells is +0; the reordering is the identity. The float32 models give exactly that."""
    import tiled_addscore_model as am
    import tiled_edge_model as em
    import tiled_esoftmax_model as sm
    from oracle.qgtc_oracle import np_pack_edges
    from reorder_model import reorder_model
    from tiled_attn_model import attention_f32, attention_grads_f32, lrelu_f32
    from tiled_float_model import aggregate_f32
    from tiled_max_model import MAX, MIN, extremum_f32, select_f32
    from tiled_sym_model import aggregate_f32_src

    e = np.zeros(0, dtype=np.int64)
    rng = np.random.default_rng(n)
    X, dY = rng.standard_normal((n, 4)).astype(np.float32), rng.standard_normal((n, 4)).astype(np.float32)
    p, q, r = (rng.standard_normal(n).astype(np.float32) for _ in range(3))
    r = np.abs(r)                                   # +0 times a negative scale is -0, by the one multiply the contract states
    zero = lambda a: a.dtype == np.float32 and not np.ascontiguousarray(a).view(np.uint32).any()      # noqa: E731  (+0, not -0)
    assert zero(aggregate_f32(e, e, n, X, transposed)) and zero(aggregate_f32_src(e, e, n, X, transposed, r, r))
    for op in (MAX, MIN):
        out, arg = extremum_f32(e, e, n, X, transposed, op)
        assert zero(out) and arg.dtype == np.int32 and (arg == -1).all() and zero(select_f32(e, e, n, dY, arg, transposed))
    Y, m, inv = attention_f32(e, e, n, X, p, q, 0.2, transposed)
    assert zero(Y) and zero(inv) and np.array_equal(m, lrelu_f32(p + np.float32(0), 0.2))
    dX, dp, dq, Dd = attention_grads_f32(e, e, n, X, p, q, dY, Y, m, inv, 0.2, transposed)
    assert zero(dX) and zero(dp) and zero(dq) and zero(Dd)
    assert em.slot_cells(e, e, n)[0].size == 0 and em.sddmm_f32(e, e, n, X, X, transposed).shape == (0,)
    assert zero(em.weighted_f32(e, e, n, X, np.zeros(0, np.float32), transposed))
    alpha, m, inv = sm.edge_softmax_f32(e, e, n, np.zeros(0, np.float32), transposed)
    assert alpha.shape == (0,) and zero(m) and zero(inv) and m.shape == (n,)
    assert sm.edge_softmax_grad_f32(e, e, n, alpha, alpha, transposed).shape == (0,)
    att = rng.standard_normal(4).astype(np.float32)
    assert am.addscore_f32(e, e, n, X, dY, att, 0.2, transposed).shape == (0,)
    assert all(zero(t) for t in am.addscore_grad_f32(e, e, n, X, dY, att, 0.2, np.zeros(0, np.float32), transposed))
    assert (em.edge_slots(e, e, n, np.array([0, -1, n]), np.array([0, 0, 0])) == -1).all()
    perm, rank = reorder_model(e, e, n)
    assert np.array_equal(perm, np.arange(n)) and np.array_equal(rank, np.arange(n))
    words = np_pack_edges(e, e, n, n, 1)
    assert words.size == (n + 7) // 8 * 8 * ((n + 127) // 128 * 4) and not words.any()


def test_the_masks_and_the_seed_do_what_the_masks_case_says(cpu_env):
    from tiled_drop_model import kept_edges, threshold
    from tiled_float_model import neighbour_lists
    from tiled_nodes_model import induced_edges

    for name in ("islands200", "g300", "g300r"):
        g = D.graph(name)
        for T in (False, True):
            rows, nbrs, row = D.mask_flags(g, T)
            assert row is not None and not rows[: 128 if T else 32].any() and rows[128 if T else 32:].all()
            deg = neighbour_lists(g.s, g.d, g.n, T)[2]
            left = neighbour_lists(*induced_edges(g.s, g.d, g.n, None, nbrs, T), g.n, T)[2]
            assert deg[row] > 0 and left[row] == 0, "the neighbour mask removes every neighbour of a live row"
        seed, lost = D.drop_seed(g)
        ks, kd = kept_edges(g.s, g.d, g.n, threshold(0.9), seed)
        deg, left = neighbour_lists(g.s, g.d, g.n, False)[2], neighbour_lists(ks, kd, g.n, False)[2]
        assert lost.size >= 1 and (deg[lost] > 0).all() and not left[lost].any() and ks.size > 0
    g = D.graph("islands200")
    rows, _, row = D.mask_flags(g, False)
    kept = induced_edges(g.s, g.d, g.n, rows, None, False)[0]
    assert (kept >= 192).all() and kept.size == 2 and rows[row], "without block 0 only the last block's two cells are left"
    inputs, run, want = D.case_masks(cpu_env, g)
    assert len(want) == 2 * 3 * (20 + 3) + 2 * 20


def test_the_comparison_sees_a_nan_only_where_the_model_has_one():
    import torch

    want = np.array([1.0, np.nan, 0.0, -0.0], dtype=np.float32)
    other_nan = np.array([0x3F800000, 0xFFC00001, 0, 0x80000000], dtype=np.uint32).view(np.float32)
    dm.same_as_model([torch.from_numpy(other_nan.copy())], [want], "another NaN's payload")
    for k, word in ((0, dm.NAN_WORD), (2, dm.SMALL_WORD), (2, 0x80000000), (3, 0), (1, 0x3F800000)):
        got = other_nan.view(np.uint32).copy()
        got[k] = word
        with pytest.raises(AssertionError, match="differs from the model in 1 of 4"):
            dm.same_as_model([torch.from_numpy(got.view(np.float32))], [want], "one wrong word")
    with pytest.raises(AssertionError, match="differs in 1 of 4"):
        dm.same_bits([torch.from_numpy(other_nan.copy())], [torch.from_numpy(want)], "bit for bit a NaN's payload counts")
    dm.same_as_model([torch.tensor([1, -2], dtype=torch.int32)], [np.array([1, 0xFFFFFFFE], dtype=np.uint32)], "words")
    with pytest.raises(AssertionError):
        dm.same_as_model([torch.tensor([1, -2], dtype=torch.int32)], [np.array([1.0, 2.0], dtype=np.float32)], "a float model")
    assert dm.signed(dm.NAN_WORD) == 0x7FC00000 and dm.signed(dm.SMALL_WORD) == -0x5A5A5A5B
