"""Mini-batch sampling on the device (qgtc_ppopp22_amd.fanout's ``sample_fanout(..., row_mask=, nbr_mask=)``, ``frontier``,
``sample_blocks``, ``sage.SAGEConv(block=)`` and the C entries of include/qgtc_blocks.h) against tests/tiled_blocks_model.py and against
the route that re-packs: ids do not change under masking, so a masked sample must be, word for word, the unmasked sample of
``pack_edges_tiled`` of the induced edges, and every sampled operator under it must give, bit for bit, what the exact models give on the
kept edges and what the plain operator gives on the adjacency packed from them - in the own form and in the nbr form (the other view,
masks swapped). No tolerance anywhere except against the dense float64 layer, which uses tests/test_tiled_fanout_gpu.py's."""
import numpy as np
import pytest

import tiled_blocks_model as bm
import tiled_drop_model as dm
import tiled_fanout_model as fm
from test_tiled_drop_gpu import _assert_all, _dev, _forwards, _grads, _inputs, _models, _np, _same
from test_tiled_fanout_gpu import KS, SWEEP
from test_tiled_float_gpu import NO_EDGES, assert_floats_identical
from tiled_attn_model import attention_grads_f32
from tiled_model import random_edges

pytestmark = pytest.mark.gpu

# n -> (seed of the graph's generator, offset of "every third node"), found on the model alone: under them every k of KS meets, on both
# axes, a masked node with deg_m > k, one with deg_m <= k and one whose unmasked degree is > k >= deg_m (asserted below before comparing).
# At n = 1 there is one node and the three cannot all exist: that case is compared without the assertion.
GRAPHS = {1: (0, 0), 97: (0, 2), 333: (1, 0), 1000: (0, 0)}
HUB_N, HUB = 5000, 2345


def _fo():
    from qgtc_ppopp22_amd import fanout

    return fanout


def _graph(n):
    """(rng, src, dst, row flags: every third node, nbr flags: a random half)"""
    seed, off = GRAPHS[n]
    rng = np.random.default_rng(seed)
    src, dst = random_edges(rng, n, 6 * n + 5)
    return rng, src, dst, np.arange(n) % 3 == off, rng.random(n) < 0.5


def _pack(torch, qgtc, src, dst, n):
    return qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)


def _bits(torch, flags):
    return None if flags is None else _dev(torch, bm.bitmap(flags))


def _sample(torch, view, k, seed, row=None, nbr=None):
    return _fo().sample_fanout(view, k, seed, row_mask=_bits(torch, row), nbr_mask=_bits(torch, nbr))


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _views(adj):
    return (("row", adj), ("col", adj.T))


# ---- 1. the masked selection -------------------------------------------------------------------------------------------------------------
def _assert_selection(torch, qgtc, adj, src, dst, n, k, seed, axis, view, row, nbr, what, repack=True):
    s = _sample(torch, view, k, seed, row, nbr)
    thr, kept = bm.thresholds_counts(src, dst, n, k, seed, axis, row, nbr)
    np.testing.assert_array_equal(_u32(s.thr), thr, err_msg=f"{what}: thr against the model")
    np.testing.assert_array_equal(_np(s.counts), kept, err_msg=f"{what}: counts against the model")
    assert s.counts.dtype == torch.int32 and s.view is view and (s.row_mask is None) == (row is None) and (s.nbr_mask is None) == (nbr is None)
    if repack:
        induced = _pack(torch, qgtc, *bm.induced_edges(src, dst, n, axis, row, nbr), n)
        again = _fo().sample_fanout(induced.T if axis == "col" else induced, k, seed)
        assert again.counts is None
        np.testing.assert_array_equal(_u32(s.thr), _u32(again.thr), err_msg=f"{what}: thr against the re-packed induced adjacency")
        assert _same(torch, s.mean_scale(), again.mean_scale()), f"{what}: 1 / kept"
    return s


@pytest.mark.parametrize("n", [1, 97, 333, 1000])
def test_the_masked_selection_equals_the_model_and_the_repacked_induced_adjacency(qgtc, n):
    import torch

    _, src, dst, row, nbr = _graph(n)
    adj = _pack(torch, qgtc, src, dst, n)
    for k in KS:
        for axis, view in _views(adj):
            if n > 1:
                degm, deg = bm.degrees_masked(src, dst, n, axis, row, nbr)[row], bm.degrees_masked(src, dst, n, axis)[row]
                assert (degm > k).any() and (degm <= k).any() and ((deg > k) & (degm <= k)).any(), (n, k, axis)
            seed = dm.SEEDS[(n + k) % 4]
            _assert_selection(torch, qgtc, adj, src, dst, n, k, seed, axis, view, row, nbr, f"n={n} k={k} {axis}")
            _assert_selection(torch, qgtc, adj, src, dst, n, k, seed, axis, view, row, None, f"n={n} k={k} {axis} rows only", repack=k == 3)
            _assert_selection(torch, qgtc, adj, src, dst, n, k, seed, axis, view, None, nbr, f"n={n} k={k} {axis} neighbours only", repack=k == 3)


def test_the_masked_selection_at_the_tile_edges(qgtc):
    """The tile-edge graph of tests/test_tiled_fanout_gpu.py - cells at rows 31 / 32 and columns 127 / 128 in rows and columns dense enough
    to be sampled - under masks that cut exactly there, each way round."""
    import torch

    n = 300
    rng = np.random.default_rng(3)
    hot, other = np.array([31, 32, 127, 128]), np.arange(n)
    src = np.concatenate([np.repeat(hot, n), np.tile(other, 4), rng.integers(0, n, 500)])
    dst = np.concatenate([np.tile(other, 4), np.repeat(hot, n), rng.integers(0, n, 500)])
    adj = _pack(torch, qgtc, src, dst, n)
    low = (other <= 31) | (other >= 128)           # keeps 31 and 128, cuts 32 .. 127
    for row, nbr in ((low, ~low), (~low, low), (low, low), (other % 2 == 1, low)):
        for k in (1, 2, 31, 127):
            for axis, view in _views(adj):
                _assert_selection(torch, qgtc, adj, src, dst, n, k, 0x0123456789ABCDEF, axis, view, row, nbr, f"tile edges k={k} {axis}",
                                  repack=k == 2)


@pytest.fixture(scope="module")
def hub():
    """n = 5000 with one full row and one full column, as tests/test_tiled_fanout_gpu.py's hub graph, but with every cell of the hub's row
    and column present exactly once (a cell listed twice is quantised away): the hub's degree is n on both axes by construction."""
    rng = np.random.default_rng(9)
    extra = random_edges(rng, HUB_N, 2 * HUB_N)
    keep = (extra[0] != HUB) & (extra[1] != HUB)
    allv, rest = np.arange(HUB_N), np.delete(np.arange(HUB_N), HUB)
    src = np.concatenate([np.full(HUB_N, HUB), rest, extra[0][keep]])
    dst = np.concatenate([allv, np.full(HUB_N - 1, HUB), extra[1][keep]])
    return rng, src, dst


@pytest.mark.parametrize("members", [40, 700, 3000])
def test_the_masked_selection_of_a_hub_takes_the_path_of_the_masked_degree(qgtc, hub, members):
    """k = 8 and neighbour masks of exactly 40, 700 and 3000 nodes: the hub is joined to every node, so its deg_m is 40 (registers), 700
    (LDS) and 3000 (the re-walk) by construction, while its unmasked degree is 5000 throughout."""
    import torch

    rng, src, dst = hub
    n, k, seed = HUB_N, 8, 1
    adj = _pack(torch, qgtc, src, dst, n)
    nbr = np.zeros(n, dtype=bool)
    nbr[np.random.default_rng(members).permutation(n)[:members]] = True
    row = (np.arange(n) % 3 == 0) | (np.arange(n) == HUB)
    for axis, view in _views(adj):
        assert bm.degrees_masked(src, dst, n, axis, row, nbr)[HUB] == members and bm.degrees_masked(src, dst, n, axis)[HUB] == n
        s = _assert_selection(torch, qgtc, adj, src, dst, n, k, seed, axis, view, row, nbr, f"hub {members} {axis}", repack=members == 700)
        who = np.nonzero(nbr)[0]
        hashes = dm.H(HUB, who, seed) if axis == "row" else dm.H(who, HUB, seed)
        assert _u32(s.thr)[HUB] == np.sort(hashes)[members - k] and int(_np(s.counts)[HUB]) == k


def test_absent_masks_give_the_unmasked_entry(qgtc):
    """NULL masks with mask_words = 0 on the C entries themselves, and all-ones bitmaps through Python: the words of qgtc_tiled_fanout_thr."""
    import torch

    from qgtc_ppopp22_amd import tiled

    n = 333
    _, src, dst, _, _ = _graph(n)
    adj = _pack(torch, qgtc, src, dst, n)
    ones = np.ones(n, dtype=bool)
    L = tiled._c_abi()
    for k in KS:
        for axis, view in _views(adj):
            want = _fo().sample_fanout(view, k, 1)
            assert want.row_mask is None and want.nbr_mask is None and want.counts is None     # today's object
            np.testing.assert_array_equal(_u32(want.thr), fm.thresholds(src, dst, n, k, 1, axis))
            fn = L.qgtc_tiled_fanout_thr_t_nodes if view.transposed else L.qgtc_tiled_fanout_thr_nodes
            for with_kept in (True, False):
                thr, kept = torch.full((n,), -1, dtype=torch.int32, device="cuda"), torch.full((n,), -1, dtype=torch.int32, device="cuda")
                tiled._c_call("selection", thr, fn, *_fo()._view_args(view), k, 1, thr.data_ptr(), n, kept.data_ptr() if with_kept else None,
                              n if with_kept else 0, None, None, 0)
                assert torch.equal(thr, want.thr)
                assert torch.equal(kept, view.degrees().clamp(max=k) if with_kept else torch.full_like(kept, -1))
            for row, nbr in ((ones, ones), (ones, None), (None, ones)):
                s = _sample(torch, view, k, 1, row, nbr)
                assert torch.equal(s.thr, want.thr) and torch.equal(s.counts, view.degrees().clamp(max=k))
                assert _same(torch, s.mean_scale(), want.mean_scale())


def test_an_adjacency_without_edges(qgtc):
    import torch

    for n in (1, 300):
        adj = _pack(torch, qgtc, *NO_EDGES, n)
        row, nbr = np.arange(n) % 2 == 0, np.ones(n, dtype=bool)
        for axis, view in _views(adj):
            s = _assert_selection(torch, qgtc, adj, *NO_EDGES, n, 2, 5, axis, view, row, nbr, f"no edges n={n}")
            assert not s.thr.any() and not s.counts.any()
            for inc in (None, row):
                got = bm.flags_of(_np(_fo().frontier(s, include=_bits(torch, inc))), n)
                np.testing.assert_array_equal(got, np.zeros(n, dtype=bool) if inc is None else inc)


# ---- 2. the frontier -----------------------------------------------------------------------------------------------------------------------
def _three_launches(torch, qgtc, s, include):
    """the route that needs no new kernel: the N = 1 sampled product of a column of ones on the other view counts, for every node, the
    sampled nodes that keep it; a compare; node_bitmap"""
    from qgtc_ppopp22_amd import tiled

    n = s.view.n
    reached = qgtc.tiledMMFloat(s.view.T, torch.ones((n, 1), device="cuda"), fanout=s).view(n) > 0
    out = tiled.node_bitmap(reached, n)
    return out if include is None else out | include


def _assert_frontier(torch, qgtc, s, src, dst, n, axis, row, nbr, what):
    fo = _fo()
    first = None
    for inc in (None, row, nbr):
        include = _bits(torch, inc)
        got = fo.frontier(s, include=include)
        assert got.dtype == torch.int32 and tuple(got.shape) == (bm.words_of(n),)
        flags = bm.flags_of(_np(got), n)           # asserts that pad bits and pad words are zero
        np.testing.assert_array_equal(flags, bm.frontier(src, dst, n, s.k, s.seed, axis, row, nbr, inc), err_msg=f"{what} against the model")
        assert torch.equal(got, _three_launches(torch, qgtc, s, include)), f"{what} against the three-launch route"
        assert torch.equal(got, fo.frontier(s, include=include)), f"{what}: two launches"
        first = flags if first is None else first
    if row is not None:
        assert torch.equal(fo.frontier(s, include=True), fo.frontier(s, include=s.row_mask))
    return first                                   # without include


@pytest.mark.parametrize("n", [97, 333, 1000])
def test_the_frontier_equals_the_model_and_the_three_launch_route(qgtc, n):
    import torch

    rng, src, dst, row, nbr = _graph(n)
    adj = _pack(torch, qgtc, src, dst, n)
    if n == 1000:                                  # 20 seeds, k = 3: a mini-batch
        row = np.zeros(n, dtype=bool)
        row[rng.permutation(n)[:20]] = True
    for k in (3,) if n == 1000 else KS:
        for axis, view in _views(adj):
            seed = dm.SEEDS[(n + k) % 4]
            for r, b in ((row, None), (row, nbr), (None, nbr)):
                _assert_frontier(torch, qgtc, _sample(torch, view, k, seed, r, b), src, dst, n, axis, r, b, f"n={n} k={k} {axis}")
            if n == 1000:
                inputs = bm.flags_of(_np(_fo().frontier(_sample(torch, view, k, seed, row), include=True)), n)
                assert not (row & ~inputs).any() and 20 < int(inputs.sum()) < n, "strictly between the seeds and all nodes"


def test_the_frontier_of_a_hub(qgtc, hub):
    """the hub keeps k = 8 of 5000 neighbours; every third node is sampled, half the nodes take part"""
    import torch

    rng, src, dst = hub
    n, k, seed = HUB_N, 8, 1
    adj = _pack(torch, qgtc, src, dst, n)
    row = (np.arange(n) % 3 == 0) | (np.arange(n) == HUB)
    nbr = np.random.default_rng(2).random(n) < 0.5
    for axis, view in _views(adj):
        _assert_frontier(torch, qgtc, _sample(torch, view, k, seed, row, nbr), src, dst, n, axis, row, nbr, f"hub {axis}")
    only = np.arange(n) == HUB
    for axis, view in _views(adj):
        flags = _assert_frontier(torch, qgtc, _sample(torch, view, k, seed, only), src, dst, n, axis, only, None, f"the hub alone {axis}")
        assert flags.sum() == k                    # the hub's k kept neighbours and nothing else


def test_an_empty_row_mask_gives_include_or_zeros(qgtc):
    import torch

    n = 333
    rng, src, dst, row, nbr = _graph(n)
    adj = _pack(torch, qgtc, src, dst, n)
    for axis, view in _views(adj):
        s = _sample(torch, view, 3, 1, np.zeros(n, dtype=bool), nbr)
        assert not s.thr.any() and not s.counts.any()
        assert not _fo().frontier(s).any() and not _fo().frontier(s, include=True).any()
        assert torch.equal(_fo().frontier(s, include=_bits(torch, row)), _bits(torch, row))
        # pad bits of include are not copied: bits from n up stay zero
        dirty = _dev(torch, np.full(bm.words_of(n), -1, dtype=np.int32))
        np.testing.assert_array_equal(bm.flags_of(_np(_fo().frontier(s, include=dirty)), n), np.ones(n, dtype=bool))


# ---- 3. the aggregates ---------------------------------------------------------------------------------------------------------------------
def _check(torch, qgtc, src, dst, n, N, k, seed, rng, row, nbr, what, repack=True):
    """both axes x both views: the sampled operators under a masked sample against the models on the kept edges and against the plain
    operators on the adjacency packed from the kept edges; then the attention's three gradients. The sample's view runs the own form,
    the other view the nbr form with the masks swapped (the Python layer's doing, inside the sample)."""
    X, dY, p, q, r, c = _inputs(rng, n, N)
    adj = _pack(torch, qgtc, src, dst, n)
    for axis, taken_on in _views(adj):
        ks, kd = bm.kept_edges(src, dst, n, k, seed, axis, row, nbr)
        kadj = _pack(torch, qgtc, ks, kd, n) if repack else None
        sample = _sample(torch, taken_on, k, seed, row, nbr)
        for transposed in (False, True):
            a = adj.T if transposed else adj
            w = f"{what} axis={axis} {'adj.T' if transposed else 'adj'} ({'own' if a is taken_on else 'nbr'}) k={k} seed={seed:#x}"
            got = _forwards(torch, qgtc, a, X, p, q, r, c, fanout=sample)
            _assert_all(got, _models(ks, kd, n, X, p, q, r, c, transposed), w + " against the model")
            if repack:
                _assert_all(got, _forwards(torch, qgtc, kadj.T if transposed else kadj, X, p, q, r, c), w + " against the re-packed adjacency")
            Y, m, inv = got[8:]
            want = attention_grads_f32(ks, kd, n, X, p, q, dY, Y, m, inv, 0.2, transposed)[:3]
            for name, g, wv in zip(("dX", "dp", "dq"), _grads(torch, qgtc, a, X, dY, p, q, r, c, "attn", fanout=sample)[1:], want):
                assert_floats_identical(g, wv, f"{w} attention {name}")


@pytest.mark.parametrize("n,N,k,seed", SWEEP, ids=[f"n{n}-N{N}-k{k}-s{dm.SEEDS.index(s)}" for n, N, k, s in SWEEP])
def test_sampled_operators_under_masks_equal_the_model_and_the_repacked_adjacency(qgtc, n, N, k, seed):
    """tests/test_tiled_fanout_gpu.py's sweep (every launcher variant of every family on both views, thinned as there), under a masked
    sample: rows every third node, neighbours a random half."""
    import torch

    rng, src, dst, row, nbr = _graph(n)
    _check(torch, qgtc, src, dst, n, N, k, seed, np.random.default_rng(17 * n + N), row, nbr, f"n={n} N={N}")


def test_one_mask_alone_and_a_hub_that_keeps_more_than_a_queue(qgtc):
    import torch

    n, N = 333, 40
    rng, src, dst, row, nbr = _graph(n)
    _check(torch, qgtc, src, dst, n, N, 3, 1, rng, row, None, "rows only")
    _check(torch, qgtc, src, dst, n, N, 3, 1, rng, None, nbr, "neighbours only")
    # hub h has 300 out-edges and 300 in-edges at n = 600; k = 40 keeps more than the 32 ids a queue holds
    n, h, k = 600, 301, 40
    rng = np.random.default_rng(4)
    others = rng.permutation(np.delete(np.arange(n, dtype=np.int64), h))[:300]
    extra = random_edges(rng, n, 2 * n)
    keep = (extra[0] != h) & (extra[1] != h)
    src = np.concatenate([np.full(300, h, np.int64), others, extra[0][keep]])
    dst = np.concatenate([others, np.full(300, h, np.int64), extra[1][keep]])
    row = (np.arange(n) % 3 == 0) | (np.arange(n) == h)
    nbr = rng.random(n) < 0.7
    _check(torch, qgtc, src, dst, n, N, k, 1, rng, row, nbr, "hub")


@pytest.mark.parametrize("mode", ["sym", "max", "attn"])
def test_tiledaggregate_gradients_under_a_masked_sample(qgtc, mode, monkeypatch):
    """The gradients equal those of the plain call on the re-packed kept adjacency, from a sample of either view; the sample is taken by
    ONE selection launch and neither the forward nor the backward takes another."""
    import torch

    n, N, k, seed = 333, 70, 3, 1
    rng, src, dst, row, nbr = _graph(n)
    X, dY, p, q, r, c = _inputs(rng, n, N)
    adj = _pack(torch, qgtc, src, dst, n)
    fo = _fo()
    launches = []
    real = fo.sample_fanout
    counted = lambda *a, **kw: (launches.append(a[1:]), real(*a, **kw))[1]
    monkeypatch.setattr(fo, "sample_fanout", counted)
    monkeypatch.setattr(fo.tiled, "sample_fanout", counted)   # where fanout=(k, seed) of the aggregates draws: fanout re-exports it
    for axis, taken_on in _views(adj):
        kadj = _pack(torch, qgtc, *bm.kept_edges(src, dst, n, k, seed, axis, row, nbr), n)
        sample = fo.sample_fanout(taken_on, k, seed, row_mask=_bits(torch, row), nbr_mask=_bits(torch, nbr))
        assert launches == [(k, seed)]
        for transposed in (False, True):
            a, ka = (adj.T, kadj.T) if transposed else (adj, kadj)
            got = _grads(torch, qgtc, a, X, dY, p, q, r, c, mode, fanout=sample)
            want = _grads(torch, qgtc, ka, X, dY, p, q, r, c, mode)
            plain = _grads(torch, qgtc, a, X, dY, p, q, r, c, mode)
            for i, (g, w, u) in enumerate(zip(got, want, plain)):
                assert (g is None) == (w is None)
                if g is not None:
                    assert_floats_identical(g, w, f"{mode} output {i} axis={axis} transposed={transposed}")
                    assert (g.view(np.uint32) != u.view(np.uint32)).any(), "the sample changes the result"
        assert launches == [(k, seed)], "no further selection launch"
        del launches[:]


# ---- 4. blocks and the layer ----------------------------------------------------------------------------------------------------------------
def _batch(n=1000, members=20):
    rng, src, dst, _, _ = _graph(n)
    seeds = np.zeros(n, dtype=bool)
    seeds[rng.permutation(n)[:members]] = True
    return rng, src, dst, seeds


def test_sample_blocks_equals_the_models_chain(qgtc):
    import torch

    n, fanouts, seed = 1000, (3, 2), 0xFEDCBA9876543210   # the layer seeds wrap past 2^64
    rng, src, dst, seeds = _batch(n)
    adj = _pack(torch, qgtc, src, dst, n)
    for axis, view in _views(adj):
        got = _fo().sample_blocks(view, _bits(torch, seeds), fanouts, seed)
        want = bm.blocks(src, dst, n, axis, seeds, fanouts, seed)
        assert len(got) == len(want) == 2
        for l, (g, w) in enumerate(zip(got, want)):
            assert isinstance(g, _fo().Block) and g.sample.view is view and g.sample.k == w["k"] and g.sample.seed == w["seed"]
            assert g.sample.row_mask is g.rows and g.sample.nbr_mask is None
            np.testing.assert_array_equal(bm.flags_of(_np(g.rows), n), w["rows"], err_msg=f"{axis} layer {l} rows")
            np.testing.assert_array_equal(bm.flags_of(_np(g.inputs), n), w["inputs"], err_msg=f"{axis} layer {l} inputs")
            np.testing.assert_array_equal(_u32(g.sample.thr), w["thr"], err_msg=f"{axis} layer {l} thr")
            np.testing.assert_array_equal(_np(g.sample.counts), w["kept"], err_msg=f"{axis} layer {l} counts")
        assert got[0].rows is got[1].inputs and torch.equal(got[1].rows, _bits(torch, seeds))


@pytest.mark.parametrize("aggr", ["mean", "max"])
def test_sageconv_on_blocks_equals_the_composition_and_the_dense_float64_definition(qgtc, aggr):
    """Two layers over sample_blocks. Bit for bit against the composition of public calls; against the dense float64 definition on the
    kept edges, on the rows of block.rows, at the tolerance tests/test_tiled_fanout_gpu.py uses for the unblocked layer
    (layers_reference.tolerances: 8 . max(max|T_f32 - T_f64|, 2^-24 . max|T_f64|), from the dense definition alone in both precisions);
    and the gradient for X reaches only rows that the first block reads, the parameters' only through rows a block keeps."""
    import torch

    import layers_reference as R
    from qgtc_ppopp22_amd import sage

    n, F_in, Hd, C, fanouts, seed = 333, 12, 10, 9, (3, 2), 7
    rng, src, dst, seeds = _batch(n, 12)
    adj = _pack(torch, qgtc, src, dst, n)
    X = rng.standard_normal((n, F_in)).astype(np.float32)
    dY = rng.standard_normal((n, C)).astype(np.float32)
    torch.manual_seed(0)
    layers = [sage.SAGEConv(F_in, Hd, aggr=aggr, fanout=5).cuda(), sage.SAGEConv(Hd, C, aggr=aggr).cuda().eval()]   # neither matters
    names = ("Y", "dX") + tuple(f"{i}.{name}" for i in range(2) for name in ("lin_self.weight", "lin_self.bias", "lin_nbr.weight"))

    def dense(dtype, axis, chain):
        x = torch.from_numpy(X).to(dtype).requires_grad_(True)
        ws, h = [], x
        for layer, b in zip(layers, chain):
            ks, kd = bm.kept_edges(src, dst, n, b["k"], b["seed"], axis, b["rows"])
            A = torch.zeros((n, n), dtype=torch.bool)
            A[torch.from_numpy(ks if axis == "row" else kd), torch.from_numpy(kd if axis == "row" else ks)] = True
            w = {name: t.detach().cpu().to(dtype).requires_grad_(True) for name, t in layer.named_parameters()}
            ws.append(w)
            if aggr == "mean":
                deg = A.sum(dim=1).to(dtype)
                agg = (A.to(dtype) @ h) * torch.where(deg > 0, 1 / deg.clamp(min=1), torch.zeros((), dtype=dtype))[:, None]
            else:
                masked = torch.where(A[:, :, None], h[None, :, :], torch.full((), -float("inf"), dtype=dtype))
                agg = torch.where(A.any(dim=1)[:, None], masked.max(dim=1).values, torch.zeros((), dtype=dtype))
            h = h @ w["lin_self.weight"].t() + w["lin_self.bias"] + agg @ w["lin_nbr.weight"].t()
        batch = torch.from_numpy(seeds)
        (h * torch.from_numpy(dY).to(dtype))[batch].sum().backward()
        grads = [w[name].grad for w in ws for name in ("lin_self.weight", "lin_self.bias", "lin_nbr.weight")]
        return dict(zip(names, [h.detach()[batch], x.grad] + grads))

    for axis, view in _views(adj):
        blocks = _fo().sample_blocks(view, _bits(torch, seeds), fanouts, seed)
        chain = bm.blocks(src, dst, n, axis, seeds, fanouts, seed)
        for layer in layers:
            layer.zero_grad()
        Xg = _dev(torch, X).requires_grad_(True)
        h = Xg
        for layer, b, w in zip(layers, blocks, chain):
            x = h.detach()
            h = layer(view, h, block=b)
            if aggr == "mean":
                agg = qgtc.tiledAggregate(view, x, b.sample.mean_scale(), fanout=b.sample)
            else:
                agg = qgtc.tiledAggregate(view, x, reduce="max", fanout=b.sample)
            assert _same(torch, h, layer.lin_self(x) + layer.lin_nbr(agg)), f"{axis}: the composition of public calls"
            assert _same(torch, h, layer(view, x, seed=99, block=b)), "the seed is ignored"
            layer.train(not layer.training)
            assert _same(torch, h, layer(view, x, block=b)), "train() / eval() make no difference"
            layer.train(not layer.training)
            outside = torch.from_numpy(~w["rows"]).cuda()
            assert outside.any() and not agg[outside].any() and _same(torch, h[outside], layer.lin_self(x)[outside]), "rows outside the block"
        batch = torch.from_numpy(seeds).cuda()
        (h * _dev(torch, dY))[batch].sum().backward()
        grads = [getattr(getattr(layer, lin), name).grad for layer in layers
                 for lin, name in (("lin_self", "weight"), ("lin_self", "bias"), ("lin_nbr", "weight"))]
        got = dict(zip(names, [h.detach()[batch], Xg.grad] + grads))
        want, want32 = dense(torch.float64, axis, chain), dense(torch.float32, axis, chain)
        tol = R.tolerances(want, want32)
        for name in names:
            err = float((got[name].detach().cpu().to(torch.float64) - want[name]).abs().max())
            print(f"{axis} {aggr} {name}: error / tolerance = {err / tol[name]:.3f} (tol {tol[name]:.3e})")
            assert tol[name] > 0 and err <= tol[name], (name, axis)
        # gradients are non-zero only through rows that a block keeps: X is read on block 0's inputs and nowhere else
        touched = (Xg.grad != 0).any(dim=1).cpu().numpy()
        assert touched.any() and not (touched & ~chain[0]["inputs"]).any()
