"""Edge dropout on the device (``edge_drop=`` of QGTC.tiledMMFloat / QGTC.tiledAggregate, conv.GCNConv / conv.GATConv and the C-ABI
_drop entries) against tests/tiled_drop_model.py: masking is dropping, so every masked operator must give, bit for bit, what the exact
models give on the kept edges and what the unmasked operator gives on ``pack_edges_tiled`` of the kept edges. Nothing is sampled and no
tolerance is used, except in the one float64 check that says so."""
import ctypes
import math

import numpy as np
import pytest

import tiled_drop_model as dm
from stream_cases import Live, capture_and_replay, eager_results, empty, env_of, ordering_probe, same, warm_adjacency
from test_tiled_float_gpu import CANARY, NAN_WORD, NO_EDGES, assert_floats_identical
from tiled_attn_model import (ATT_FORWARD_VARIANTS, ATT_GRAD_VARIANTS, ATT_TRANSPOSED_VARIANTS, att_grad_variant, att_variant, attention_f32,
                              attention_grads_f32, lrelu_f32)
from tiled_float_model import FLOAT_FORWARD_VARIANTS, FLOAT_TRANSPOSED_VARIANTS, float_variant, neighbour_lists
from tiled_max_model import MAX, MAX_FORWARD_VARIANTS, MAX_TRANSPOSED_VARIANTS, MIN, extremum_f32, max_variant
from tiled_model import random_edges, set_cells
from tiled_sym_model import aggregate_f32_src

pytestmark = pytest.mark.gpu

SWEEP_N = (1, 16, 17, 33, 65, 129, 257)
SWEEP_n = (97, 333, 1000)                          # n % 32 and n % 128 are nonzero
RATES = (0.0, 0.1, 0.6, 1.0 - 2.0 ** -32)          # thresholds 0, 429496729, 2576980377, 2^32 - 1
# the grid N x n x both views x rate x seed, thinned: every (n, N) runs both views under one rate and one seed, which rotate
SWEEP = [(n, N, RATES[(iN + i) % 4], dm.SEEDS[(2 * iN + i) % 4]) for iN, N in enumerate(SWEEP_N) for i, n in enumerate(SWEEP_n)]


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _same(torch, a, b):
    return torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32))


def _inputs(rng, n, N):
    X, dY = rng.standard_normal((n, N)).astype(np.float32), rng.standard_normal((n, N)).astype(np.float32)
    p, q = rng.uniform(-1, 1, n).astype(np.float32), rng.uniform(-1, 1, n).astype(np.float32)
    r, c = rng.uniform(0.5, 2.0, n).astype(np.float32), rng.uniform(0.5, 2.0, n).astype(np.float32)
    return X, dY, p, q, r, c


def _forwards(torch, qgtc, a, X, p, q, r, c, **kw):
    """every forward of the public interface on view `a`, as NumPy: sum, row scale, both scales, max + arg, min + arg, attention + stats"""
    X, p, q, r, c = (_dev(torch, t) for t in (X, p, q, r, c))
    mx, amx = qgtc.tiledMMFloat(a, X, reduce="max", return_arg=True, **kw)
    mn, amn = qgtc.tiledMMFloat(a, X, reduce="min", return_arg=True, **kw)
    assert _same(torch, qgtc.tiledMMFloat(a, X, reduce="max", **kw), mx)
    att = qgtc.tiledMMFloat(a, X, attn=(p, q), return_stats=True, **kw)
    res = (qgtc.tiledMMFloat(a, X, **kw), qgtc.tiledMMFloat(a, X, r, **kw), qgtc.tiledMMFloat(a, X, r, c, **kw),
           qgtc.tiledMMFloat(a, X, None, c, **kw), mx, amx, mn, amn) + tuple(att)
    return tuple(_np(t) for t in res)


NAMES = ("sum", "row scale", "both scales", "source scale", "max", "argmax", "min", "argmin", "attention", "m", "inv")


def _models(src, dst, n, X, p, q, r, c, transposed):
    mx, amx = extremum_f32(src, dst, n, X, transposed, MAX)
    mn, amn = extremum_f32(src, dst, n, X, transposed, MIN)
    return (aggregate_f32_src(src, dst, n, X, transposed), aggregate_f32_src(src, dst, n, X, transposed, r),
            aggregate_f32_src(src, dst, n, X, transposed, r, c), aggregate_f32_src(src, dst, n, X, transposed, None, c),
            mx, amx, mn, amn) + attention_f32(src, dst, n, X, p, q, 0.2, transposed)


def _assert_all(got, want, what):
    assert len(got) == len(want) == len(NAMES)
    for name, g, w in zip(NAMES, got, want):
        if g.dtype == np.int32:
            np.testing.assert_array_equal(g, w, err_msg=f"{what} {name}")
        else:
            assert_floats_identical(g, w, f"{what} {name}")


def _check(torch, qgtc, src, dst, n, N, rate, seed, rng, what, adj=None, repack=True):
    """both views under (rate, seed): the masked operators on `adj` against the models on the kept edges and, with `repack`, against the
    unmasked operators on the adjacency packed from the kept edges"""
    X, dY, p, q, r, c = _inputs(rng, n, N)
    ks, kd = dm.kept_edges(src, dst, n, dm.threshold(rate), seed)
    adj = adj if adj is not None else qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    kadj = qgtc.pack_edges_tiled(_dev(torch, ks), _dev(torch, kd), n) if repack else None
    for transposed in (False, True):
        a = adj.T if transposed else adj
        w = f"{what} {'adj.T' if transposed else 'adj'} rate={rate} seed={seed:#x}"
        got = _forwards(torch, qgtc, a, X, p, q, r, c, edge_drop=(rate, seed))
        _assert_all(got, _models(ks, kd, n, X, p, q, r, c, transposed), w + " against the model")
        if repack:
            _assert_all(got, _forwards(torch, qgtc, kadj.T if transposed else kadj, X, p, q, r, c), w + " against the re-packed adjacency")
        # the attention gradients run the masked backward product and both masked score-gradient walks at this width
        Y, m, inv = got[8:]
        want = attention_grads_f32(ks, kd, n, X, p, q, dY, Y, m, inv, 0.2, transposed)[:3]
        for name, g, wv in zip(("dX", "dp", "dq"), _grads(torch, qgtc, a, X, dY, p, q, r, c, "attn", edge_drop=(rate, seed))[1:], want):
            assert_floats_identical(g, wv, f"{w} attention {name}")
    return adj, (ks, kd), (X, dY, p, q, r, c)


# ---- 1. the sweep ---------------------------------------------------------------------------------------------------------------------------
def test_the_sweep_reaches_every_launcher_variant():
    """Against the models' copies of the launchers' switches: the entries of qgtc_tiled_float_drop.hip, qgtc_tiled_float_t_drop.hip,
    qgtc_tiled_max_drop.hip, qgtc_tiled_attn_drop.hip and qgtc_tiled_attn_t_drop.hip go through their parents' launchers (one per kernel
    family, at the foot of its tiled_*_kernels.hip.h), so they choose as their parents do. Every case runs the plain
    sum, each scale alone and both (all four packs of the float kernels), max and min, and the attention forward on both views."""
    for transposed, fl, mx, at in ((False, FLOAT_FORWARD_VARIANTS, MAX_FORWARD_VARIANTS, ATT_FORWARD_VARIANTS),
                                   (True, FLOAT_TRANSPOSED_VARIANTS, MAX_TRANSPOSED_VARIANTS, ATT_TRANSPOSED_VARIANTS)):
        assert sorted({float_variant(N, transposed) for N in SWEEP_N}) == sorted(fl)
        assert sorted({max_variant(N, transposed) for N in SWEEP_N}) == sorted(mx)
        assert sorted({att_variant(N, transposed) for N in SWEEP_N}) == sorted(at)
    assert len(SWEEP) == 21 and {s[0] for s in SWEEP} == set(SWEEP_n) and {s[1] for s in SWEEP} == set(SWEEP_N)
    assert {s[2] for s in SWEEP} == set(RATES) and {s[3] for s in SWEEP} == set(dm.SEEDS)
    assert [dm.threshold(r) for r in RATES] == [0, 429496729, 2576980377, 2 ** 32 - 1]
    for rate in RATES:                             # every rate meets every n, and a narrow, a middle and a wide output
        assert {s[0] for s in SWEEP if s[2] == rate} == set(SWEEP_n)
        assert len({s[1] for s in SWEEP if s[2] == rate}) >= 5
    for N in SWEEP_N:                              # every output width runs under three of the four rates
        assert len({s[2] for s in SWEEP if s[1] == N}) == 3
    assert sorted({att_grad_variant(N) for N in SWEEP_N}) == sorted(ATT_GRAD_VARIANTS)   # every case also runs the attention backward


@pytest.mark.parametrize("n,N,rate,seed", SWEEP, ids=[f"n{n}-N{N}-r{RATES.index(r)}-s{dm.SEEDS.index(s)}" for n, N, r, s in SWEEP])
def test_masked_operators_equal_the_model_and_the_repacked_adjacency(qgtc, n, N, rate, seed):
    import torch

    rng = np.random.default_rng(17 * n + N)
    src, dst = random_edges(rng, n, 6 * n + 5)
    _check(torch, qgtc, src, dst, n, N, rate, seed, rng, f"n={n} N={N}")


# ---- 2. special cases ---------------------------------------------------------------------------------------------------------------------
def test_rate_zero_is_the_plain_call(qgtc):
    import torch

    n, N = 333, 70
    rng = np.random.default_rng(2)
    src, dst = random_edges(rng, n, 6 * n + 5)
    X, dY, p, q, r, c = _inputs(rng, n, N)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    for a in (adj, adj.T):
        plain = _forwards(torch, qgtc, a, X, p, q, r, c)
        for seed in dm.SEEDS:
            _assert_all(_forwards(torch, qgtc, a, X, p, q, r, c, edge_drop=(0.0, seed)), plain, f"rate 0 seed {seed:#x}")
        _assert_all(_forwards(torch, qgtc, a, X, p, q, r, c, edge_drop=None), plain, "edge_drop=None")


def test_a_hub_keeps_more_than_a_queue(qgtc):
    """Hub h has 300 out-edges and 300 in-edges at n = 600; at rate 0.5 more than 32 of each survive, so its queue flushes mid-row with
    dropped neighbours in between."""
    import torch

    n, h, N, rate, seed = 600, 301, 40, 0.5, 1
    rng = np.random.default_rng(4)
    others = rng.permutation(np.delete(np.arange(n, dtype=np.int64), h))[:300]
    extra = random_edges(rng, n, 2 * n)
    keep = (extra[0] != h) & (extra[1] != h)
    src = np.concatenate([np.full(300, h, np.int64), others, extra[0][keep]])
    dst = np.concatenate([others, np.full(300, h, np.int64), extra[1][keep]])
    ks, kd = dm.kept_edges(src, dst, n, dm.threshold(rate), seed)
    out_kept, in_kept = int((ks == h).sum()), int((kd == h).sum())
    assert 32 < out_kept < 300 and 32 < in_kept < 300, (out_kept, in_kept)
    _check(torch, qgtc, src, dst, n, N, rate, seed, rng, "hub")


def test_a_row_that_loses_every_neighbour(qgtc):
    import torch

    n, N, rate, seed = 333, 33, 0.6, 0x0123456789ABCDEF
    rng = np.random.default_rng(8)
    src, dst = random_edges(rng, n, 3 * n)
    ks, kd = dm.kept_edges(src, dst, n, dm.threshold(rate), seed)
    adj, _, (X, dY, p, q, r, c) = _check(torch, qgtc, src, dst, n, N, rate, seed, rng, "lost rows")
    for transposed in (False, True):
        _, _, deg = neighbour_lists(src, dst, n, transposed)
        _, _, kdeg = neighbour_lists(ks, kd, n, transposed)
        lost = (deg > 0) & (kdeg == 0)
        assert lost.any(), "some row with neighbours loses all of them"
        got = _forwards(torch, qgtc, adj.T if transposed else adj, X, p, q, r, c, edge_drop=(rate, seed))
        for name, g in zip(NAMES, got):
            if name in ("argmax", "argmin"):
                assert (g[lost] == -1).all(), name
            elif name == "m":
                assert_floats_identical(g[lost], lrelu_f32(p[lost], 0.2), "m of a row without neighbours is L(p)")
            else:
                assert (g[lost].view(np.uint32) == 0).all(), name      # +0, and inv = 0


def test_a_hash_equal_to_the_threshold_is_kept(qgtc):
    """H >= T, not H > T: with T the hash of one set cell (any T is the rate T / 2^32) that cell stays."""
    import torch

    n, N, seed = 97, 5, 1
    rng = np.random.default_rng(12)
    src, dst = random_edges(rng, n, 4 * n)
    cells = set_cells(src, dst, n)
    i, j = int(cells[7] // n), int(cells[7] % n)
    T = int(dm.H(i, j, seed))
    rate = T / 2.0 ** 32
    assert dm.threshold(rate) == T and 0 < rate < 1
    ks, kd = dm.kept_edges(src, dst, n, T, seed)
    assert ((ks == i) & (kd == j)).any() and not dm.kept(i, j, seed, T, ">")
    _check(torch, qgtc, src, dst, n, N, rate, seed, rng, "boundary")


@pytest.mark.parametrize("n,N,loop", [(1, 1, False), (1, 5, True), (300, 24, False)])
def test_an_empty_adjacency_and_one_node(qgtc, n, N, loop):
    import torch

    rng = np.random.default_rng(n + N)
    src, dst = (np.zeros(1, np.int64), np.zeros(1, np.int64)) if loop else NO_EDGES
    # H(0, 0, seed 0) = 0x01fce552: rate 0.1 drops the loop of node 0 under seed 0 and keeps it under seed 1
    for seed in (0, 1):
        ks, _ = dm.kept_edges(src, dst, n, dm.threshold(0.1), seed)
        assert ks.size == (1 if loop and seed == 1 else 0)
        _check(torch, qgtc, src, dst, n, N, 0.1, seed, rng, f"n={n} loop={loop}")


def test_a_reordered_adjacency(qgtc):
    """The mask is in the adjacency's own numbering: the model hashes the NEW ids."""
    import torch

    n, N, rate, seed = 1000, 40, 0.1, 2 ** 64 - 1
    rng = np.random.default_rng(31)
    src, dst = random_edges(rng, n, 6 * n + 5)
    re = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n, reorder=True)
    rank = re.rank.cpu().numpy()
    assert (rank != np.arange(n)).any()
    _check(torch, qgtc, rank[src], rank[dst], n, N, rate, seed, rng, "reordered", adj=re, repack=False)
    old = dm.kept_edges(src, dst, n, dm.threshold(rate), seed)
    new = dm.kept_edges(rank[src], rank[dst], n, dm.threshold(rate), seed)
    inv_rank = np.argsort(rank)
    assert set(zip(old[0].tolist(), old[1].tolist())) != set(zip(inv_rank[new[0]].tolist(), inv_rank[new[1]].tolist()))


# ---- 3. backward ----------------------------------------------------------------------------------------------------------------------------
def _grads(torch, qgtc, a, X, dY, p, q, r, c, mode, needs=(True, True, True), **kw):
    Xg = _dev(torch, X).requires_grad_(needs[0])
    pg, qg = _dev(torch, p).requires_grad_(needs[1]), _dev(torch, q).requires_grad_(needs[2])
    if mode == "sym":
        Y = qgtc.tiledAggregate(a, Xg, _dev(torch, r), _dev(torch, c), **kw)
    elif mode == "max":
        Y = qgtc.tiledAggregate(a, Xg, reduce="max", **kw)
    else:
        Y = qgtc.tiledAggregate(a, Xg, attn=(pg, qg), **kw)
    Y.backward(_dev(torch, dY))
    return [_np(Y)] + [None if t.grad is None else _np(t.grad) for t in (Xg, pg, qg)]


@pytest.mark.parametrize("mode", ["sym", "max", "attn"])
def test_backward_equals_the_unmasked_composition_on_the_repacked_adjacency(qgtc, mode):
    import torch

    n, N, rate, seed = 333, 70, 0.6, 1
    rng = np.random.default_rng(5)
    src, dst = random_edges(rng, n, 6 * n + 5)
    X, dY, p, q, r, c = _inputs(rng, n, N)
    ks, kd = dm.kept_edges(src, dst, n, dm.threshold(rate), seed)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    kadj = qgtc.pack_edges_tiled(_dev(torch, ks), _dev(torch, kd), n)
    subsets = [(bool(m & 1), bool(m & 2), bool(m & 4)) for m in range(1, 8)] if mode == "attn" else [(True, False, False)]
    for a, ka in ((adj, kadj), (adj.T, kadj.T)):
        for needs in subsets:
            got = _grads(torch, qgtc, a, X, dY, p, q, r, c, mode, needs, edge_drop=(rate, seed))
            want = _grads(torch, qgtc, ka, X, dY, p, q, r, c, mode, needs)
            plain = _grads(torch, qgtc, a, X, dY, p, q, r, c, mode, needs)
            for k, (g, w, u) in enumerate(zip(got, want, plain)):
                assert (g is None) == (w is None) and (g is None) == (k > 0 and not needs[k - 1]), (needs, k)
                if g is not None:
                    assert_floats_identical(g, w, f"{mode} {needs} output {k} transposed={a.transposed}")
                    assert (g.view(np.uint32) != u.view(np.uint32)).any(), "the mask changes the result"
    if mode == "attn":                             # ... and the model of the gradients on the kept edges
        Y, m, inv = attention_f32(ks, kd, n, X, p, q, 0.2, False)
        dX, dp, dq, _ = attention_grads_f32(ks, kd, n, X, p, q, dY, Y, m, inv, 0.2, False)
        got = _grads(torch, qgtc, adj, X, dY, p, q, r, c, mode, edge_drop=(rate, seed))
        for g, w, name in zip(got, (Y, dX, dp, dq), ("Y", "dX", "dp", "dq")):
            assert_floats_identical(g, w, f"model {name}")
    assert not qgtc.tiledAggregate(adj, _dev(torch, X), edge_drop=(rate, seed)).requires_grad


def test_masked_attention_against_a_dense_float64_softmax(qgtc):
    """The one comparison with a tolerance: forward and gradients of the masked attention against a float64 masked softmax on the dense
    adjacency, differentiated by torch.autograd, with the mask applied to the dense matrix cell by cell. The bound is that of
    tests/test_tiled_attn_model.py for scores in [-1, 1]: (d_max + ceil(N / 64) + 40) 2^-24 times the float64 sum of the absolute terms."""
    import torch

    n, N, rate, seed, slope = 97, 17, 0.5, 0x0123456789ABCDEF, 0.2
    rng = np.random.default_rng(7 * n + N)
    src, dst = random_edges(rng, n, 6 * n + 5)
    X, dY, p, q, r, c = _inputs(rng, n, N)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    cells = set_cells(src, dst, n)
    dense = np.zeros((n, n), bool)
    dense[cells // n, cells % n] = True
    gi, gj = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    dense &= dm.kept(gi, gj, seed, dm.threshold(rate))
    assert 0 < dense.sum() < cells.size
    for transposed in (False, True):
        A = torch.from_numpy(dense.T.copy() if transposed else dense)
        Xt, pt, qt = (torch.from_numpy(t.astype(np.float64)).requires_grad_(True) for t in (X, p, q))
        logits = torch.nn.functional.leaky_relu(pt[:, None] + qt[None, :], slope)
        logits = torch.where(A, logits, torch.full((), -float("inf"), dtype=torch.float64))
        alpha = torch.where(A.any(dim=1)[:, None], torch.softmax(logits, dim=1), torch.zeros((), dtype=torch.float64))
        Y = alpha @ Xt
        Y.backward(torch.from_numpy(dY.astype(np.float64)))
        alpha = alpha.detach().numpy()
        got = _grads(torch, qgtc, adj.T if transposed else adj, X, dY, p, q, r, c, "attn", negative_slope=slope, edge_drop=(rate, seed))
        d_max = int(max(dense.sum(axis=0).max(), dense.sum(axis=1).max()))
        bound = (d_max + math.ceil(N / 64) + 40) * 2.0 ** -24
        aX, adY = np.abs(X.astype(np.float64)), np.abs(dY.astype(np.float64))
        edge = alpha * (adY @ aX.T + (adY * (alpha @ aX)).sum(axis=1)[:, None])
        checks = (("Y", got[0], Y.detach().numpy(), alpha @ aX), ("dX", got[1], Xt.grad.numpy(), alpha.T @ adY),
                  ("dp", got[2], pt.grad.numpy(), edge.sum(axis=1)), ("dq", got[3], qt.grad.numpy(), edge.sum(axis=0)))
        for name, g, want, mag in checks:
            err = np.abs(g.astype(np.float64) - want)
            print(f"transposed={transposed} {name}: worst error / bound = {float((err / np.maximum(bound * mag, 1e-300)).max()):.4f}")
            assert (err <= bound * mag).all(), (name, transposed)
            assert np.abs(want).max() > 0


# ---- 4. launch behaviour --------------------------------------------------------------------------------------------------------------------
def test_two_launches_agree_and_two_seeds_differ(qgtc):
    import torch

    n, N = 1000, 96
    rng = np.random.default_rng(6)
    src, dst = random_edges(rng, n, 6 * n + 5)
    X, dY, p, q, r, c = _inputs(rng, n, N)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    for a in (adj, adj.T):
        first, again, other = (_forwards(torch, qgtc, a, X, p, q, r, c, edge_drop=(0.5, s)) for s in (1, 1, 1 + 2 ** 32))
        for name, f, g, o in zip(NAMES, first, again, other):
            assert (f.view(np.uint32) == g.view(np.uint32)).all(), name
            assert (f.view(np.uint32) != o.view(np.uint32)).any(), name


def _live(env, transposed):
    """Masked forward and backward of all three modes as a ``Live`` case of tests/stream_cases.py: X, dY, p and q are the contents, ONE
    pair of scales and ONE seed stay (a captured graph replays one mask); the reference is the eager result on the default stream.
    ``live.both_ways(edge_drop)`` runs the same on the buffers under another pair."""
    torch, qgtc = env.torch, env.Q
    n, N, drop = 600, 40, (0.5, 0x0123456789ABCDEF)
    rng = np.random.default_rng(41)
    src, dst = random_edges(rng, n, 6 * n + 5)
    adj = warm_adjacency(env, src, dst, n)
    a = adj.T if transposed else adj
    data = [_inputs(rng, n, N) for _ in range(4)]      # (X, dY, p, q, r, c)
    r, c = _dev(torch, data[0][4]), _dev(torch, data[0][5])
    contents = [d[:4] for d in data]
    X, dY, p, q = bufs = [empty(env, t.shape, torch.float32) for t in contents[0]]
    for t in (X, p, q):
        t.requires_grad_(True)

    def both_ways(edge_drop=drop):
        Ys = qgtc.tiledAggregate(a, X, r, c, edge_drop=edge_drop)
        Ym = qgtc.tiledAggregate(a, X, reduce="max", edge_drop=edge_drop)
        Ya = qgtc.tiledAggregate(a, X, attn=(p, q), edge_drop=edge_drop)
        grads = torch.autograd.grad(Ys, X, dY) + torch.autograd.grad(Ym, X, dY) + torch.autograd.grad(Ya, (X, p, q), dY)
        return [Ys.detach(), Ym.detach(), Ya.detach(), *grads]

    live = Live(torch, bufs, contents, eager_results(torch, bufs, contents, both_ways), run=both_ways, keep=adj)
    live.both_ways = both_ways
    return live


@pytest.mark.parametrize("transposed", [False, True], ids=["adj", "adjT"])
def test_side_stream_and_graph_capture(qgtc, oracle, transposed):
    """Masked forward and backward of all three modes behind a timed head start on three fresh side streams (``ordering_probe``) and
    captured into a graph; three replays on new inputs equal the eager results under the captured seed (``capture_and_replay``).
    Another seed gives other results."""
    import torch

    live = _live(env_of(qgtc, oracle, torch), transposed)
    what = f"edge dropout, {'adj.T' if transposed else 'adj'}"
    ordering_probe(torch, qgtc, live, what)
    capture_and_replay(torch, qgtc, live, what)
    live.load(3)
    other = [t.cpu() for t in live.both_ways(edge_drop=(0.5, 7))]
    assert not any(same(x, e) for x, e in zip(other[:3], live.expected[3][:3]))


# ---- 5. the C entries write what they own and nothing else -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n,N", [(97, 17), (333, 129)])
def test_the_c_entries_stay_within_their_outputs(qgtc, n, N):
    import torch

    from qgtc_ppopp22_amd import cabi

    L = cabi.load()
    rate, seed = 0.6, 2 ** 64 - 1
    T = dm.threshold(rate)
    rng = np.random.default_rng(n)
    src, dst = random_edges(rng, n, 6 * n + 5)
    X, dY, p, q, r, c = _inputs(rng, n, N)
    ks, kd = dm.kept_edges(src, dst, n, T, seed)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    dX_, ddY, dp_, dq_, dr_, dc_ = (_dev(torch, t) for t in (X, dY, p, q, r, c))
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fresh(elems, dtype=torch.float32):
        if dtype == torch.int32:
            return torch.full((elems + CANARY,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        return torch.full((elems + CANARY,), float("nan"), dtype=torch.float32, device="cuda")

    def taken(buf, elems):
        a = buf.cpu().numpy()
        assert (a[elems:].view(np.uint32) == (0x5A5A5A5A if a.dtype == np.int32 else NAN_WORD)).all(), "canaries"
        return a[:elems]

    for transposed in (False, True):
        t = adj.T
        idx = (t.col_ptr.data_ptr(), t.col_tile.data_ptr(), t.col_rb.data_ptr(), adj.tiles.data_ptr()) if transposed else \
            (adj.row_ptr.data_ptr(), adj.kquad.data_ptr(), adj.tiles.data_ptr())
        sfx = "_t_drop" if transposed else "_drop"
        want = dict(zip(NAMES, _models(ks, kd, n, X, p, q, r, c, transposed)))
        for name, rs, cs in (("sum", None, None), ("row scale", dr_, None), ("both scales", dr_, dc_), ("source scale", None, dc_)):
            out = fresh(n * N)
            rc = getattr(L, "qgtc_tiledmm_f32" + sfx)(*idx, adj.n_tiles, n, dX_.data_ptr(), n * N, N, rs.data_ptr() if rs is not None else None,
                                                      cs.data_ptr() if cs is not None else None, out.data_ptr(), n * N, T, seed, st)
            assert rc == 0
            assert_floats_identical(taken(out, n * N).reshape(n, N), want[name], "C " + name)
        for op, name in ((0, "max"), (1, "min")):
            out, arg = fresh(n * N), fresh(n * N, torch.int32)
            rc = getattr(L, "qgtc_tiledmax_f32" + sfx)(*idx, adj.n_tiles, n, dX_.data_ptr(), n * N, N, op, out.data_ptr(), n * N, arg.data_ptr(),
                                                       n * N, T, seed, st)
            assert rc == 0
            assert_floats_identical(taken(out, n * N).reshape(n, N), want[name], "C " + name)
            np.testing.assert_array_equal(taken(arg, n * N).reshape(n, N), want["arg" + name])
            out = fresh(n * N)                    # without arg
            rc = getattr(L, "qgtc_tiledmax_f32" + sfx)(*idx, adj.n_tiles, n, dX_.data_ptr(), n * N, N, op, out.data_ptr(), n * N, None, 0, T,
                                                       seed, st)
            assert rc == 0
            assert_floats_identical(taken(out, n * N).reshape(n, N), want[name], "C " + name + " without arg")
        # the attention forward from the MASKED maximum of the neighbours' scores
        M = fresh(n)
        rc = getattr(L, "qgtc_tiledmax_f32" + sfx)(*idx, adj.n_tiles, n, dq_.data_ptr(), n, 1, 0, M.data_ptr(), n, None, 0, T, seed, st)
        assert rc == 0
        taken(M, n)
        Y, m, inv = want["attention"], want["m"], want["inv"]
        out, mo, io = fresh(n * N), fresh(n), fresh(n)
        rc = getattr(L, "qgtc_tiledatt_f32" + sfx)(*idx, adj.n_tiles, n, dX_.data_ptr(), n * N, N, dp_.data_ptr(), dq_.data_ptr(), 0.2, 0,
                                                   M.data_ptr(), mo.data_ptr(), io.data_ptr(), out.data_ptr(), n * N, T, seed, st)
        assert rc == 0
        assert_floats_identical(taken(out, n * N).reshape(n, N), Y, "C forward")
        assert_floats_identical(taken(mo, n), m, "C m")
        assert_floats_identical(taken(io, n), inv, "C inv")
        gX, gp, gq, Dm = attention_grads_f32(ks, kd, n, X, p, q, dY, Y, m, inv, 0.2, transposed)
        dm_, di_, D = _dev(torch, m), _dev(torch, inv), _dev(torch, Dm)
        g = fresh(n)
        rc = getattr(L, "qgtc_tiledatt_grad_f32" + sfx)(*idx, adj.n_tiles, n, ddY.data_ptr(), dX_.data_ptr(), n * N, N, dp_.data_ptr(),
                                                        dq_.data_ptr(), 0.2, 0, dm_.data_ptr(), di_.data_ptr(), D.data_ptr(), g.data_ptr(), n,
                                                        T, seed, st)
        assert rc == 0
        assert_floats_identical(taken(g, n), gp, "C dp")
        # the other two gradients of the forward on the OTHER view run on this one: its dX and dq
        Yo, m_o, inv_o = attention_f32(ks, kd, n, X, p, q, 0.2, not transposed)
        gXo, _, gqo, Do = attention_grads_f32(ks, kd, n, X, p, q, dY, Yo, m_o, inv_o, 0.2, not transposed)
        dmo, dio, Dod = _dev(torch, m_o), _dev(torch, inv_o), _dev(torch, Do)
        out = fresh(n * N)
        rc = getattr(L, "qgtc_tiledatt_f32" + sfx)(*idx, adj.n_tiles, n, ddY.data_ptr(), n * N, N, dq_.data_ptr(), dp_.data_ptr(), 0.2, 1,
                                                   dmo.data_ptr(), None, dio.data_ptr(), out.data_ptr(), n * N, T, seed, st)
        assert rc == 0
        assert_floats_identical(taken(out, n * N).reshape(n, N), gXo, "C dX")
        g = fresh(n)
        rc = getattr(L, "qgtc_tiledatt_grad_f32" + sfx)(*idx, adj.n_tiles, n, dX_.data_ptr(), ddY.data_ptr(), n * N, N, dq_.data_ptr(),
                                                        dp_.data_ptr(), 0.2, 1, dmo.data_ptr(), dio.data_ptr(), Dod.data_ptr(), g.data_ptr(), n,
                                                        T, seed, st)
        assert rc == 0
        assert_floats_identical(taken(g, n), gqo, "C dq")
    torch.cuda.synchronize()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals(qgtc):
    import torch

    n, N = 97, 8
    rng = np.random.default_rng(3)
    src, dst = random_edges(rng, n, 4 * n)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    X, dY, p, q, r, c = (_dev(torch, t) for t in _inputs(rng, n, N))
    calls = [lambda **kw: qgtc.tiledMMFloat(adj, X, **kw), lambda **kw: qgtc.tiledMMFloat(adj.T, X, r, c, **kw),
             lambda **kw: qgtc.tiledMMFloat(adj, X, reduce="max", return_arg=True, **kw),
             lambda **kw: qgtc.tiledMMFloat(adj, X, attn=(p, q), return_stats=True, **kw),
             lambda **kw: qgtc.tiledAggregate(adj, X, **kw), lambda **kw: qgtc.tiledAggregate(adj, X, reduce="min", **kw),
             lambda **kw: qgtc.tiledAggregate(adj.T, X, attn=(p, q), **kw)]
    for call in calls:
        for rate in (-0.1, 1.0, 1.5, float("nan"), float("inf"), -float("inf")):
            with pytest.raises(ValueError, match="rate"):
                call(edge_drop=(rate, 0))
        for seed in (-1, 2 ** 64, -2 ** 63):
            with pytest.raises(ValueError, match="seed"):
                call(edge_drop=(0.5, seed))
        for bad in (0.5, (0.5,), (0.5, 1, 2), "ab", {0.5: 1}, torch.tensor([0.5, 1.0])):
            with pytest.raises(TypeError, match="pair"):
                call(edge_drop=bad)
        for bad in ((0.5, 1.0), (0.5, None), ("0.5", 1), (None, 1), (0.5, True)):
            with pytest.raises(TypeError):
                call(edge_drop=bad)
        call(edge_drop=(0, 0))                     # an int rate 0 and the lists' form are pairs too
        call(edge_drop=[0.999, 2 ** 64 - 1])
    from qgtc_ppopp22_amd import conv

    for bad in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError, match="edge_drop"):
            conv.GCNConv(4, 4, 4, edge_drop=bad)
        with pytest.raises(ValueError, match="edge_drop"):
            conv.GATConv(4, 4, edge_drop=bad)
    layer = conv.GCNConv(N, 4, 4, edge_drop=0.5).cuda()
    with pytest.raises(NotImplementedError, match="TiledAdjacency"):
        layer(torch.eye(n, device="cuda"), X)
    layer.eval()
    layer(torch.eye(n, device="cuda"), X)          # eval mode has no mask: the dense route is the one it was


# ---- 7. the layers --------------------------------------------------------------------------------------------------------------------------
def _graph(torch, qgtc, n, seed):
    rng = np.random.default_rng(seed)
    src, dst = random_edges(rng, n, 6 * n + 5)
    return qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n), rng


@pytest.mark.parametrize("norm,aggr", [(None, "sum"), ("mean", "sum"), ("sym", "sum"), (None, "max")])
def test_gcnconv_under_the_mask(qgtc, norm, aggr):
    import torch

    from qgtc_ppopp22_amd import conv

    n, F_in, H, C, rate, seed = 333, 12, 20, 7, 0.5, 0x0123456789ABCDEF
    adj, rng = _graph(torch, qgtc, n, 21)
    X = _dev(torch, rng.standard_normal((n, F_in)).astype(np.float32))
    torch.manual_seed(0)
    layer = conv.GCNConv(F_in, H, C, norm=norm, aggr=aggr, edge_drop=rate).cuda()
    plain = conv.GCNConv(F_in, H, C, norm=norm, aggr=aggr).cuda()
    plain.load_state_dict(layer.state_dict())
    assert layer.training and layer.keep_scale == 2.0
    drop = (rate, seed)
    if aggr == "max":
        agg = lambda Z: qgtc.tiledAggregate(adj, Z, reduce="max", edge_drop=drop)  # noqa: E731
    else:
        row = {None: None, "mean": adj.mean_scale(), "sym": adj.sym_scale()}[norm]
        row = torch.full((n,), 2.0, device="cuda") if row is None else row * 2.0    # fl(1 / (1 - 0.5)) = 2
        src_scale = adj.T.sym_scale() if norm == "sym" else None
        agg = lambda Z: qgtc.tiledAggregate(adj, Z, row, src_scale, edge_drop=drop)  # noqa: E731
    want = agg(torch.mm(agg(torch.mm(X, layer.W_in)), layer.W_out))
    got = layer(adj, X, edge_seed=seed)
    assert _same(torch, got, want)
    assert not _same(torch, got, layer(adj, X, edge_seed=seed + 1))
    # a drawn seed follows torch's CPU generator, and both aggregates share it
    torch.manual_seed(5)
    a = layer(adj, X)
    torch.manual_seed(5)
    hi, lo = torch.randint(0, 1 << 32, (2,), dtype=torch.int64).tolist()
    assert _same(torch, a, layer(adj, X, edge_seed=(hi << 32) | lo))
    assert not _same(torch, a, layer(adj, X))      # the next forward draws the next seed
    # eval: the layer as it is without the keyword, bit for bit
    layer.eval()
    assert _same(torch, layer(adj, X), plain(adj, X)) and _same(torch, layer(adj, X, edge_seed=seed), plain(adj, X))
    # one SGD step
    layer.train()
    before = [w.detach().clone() for w in layer.parameters()]
    opt = torch.optim.SGD(layer.parameters(), lr=1e-3)
    loss = layer(adj, X, edge_seed=seed).square().mean()
    loss.backward()
    assert all(w.grad is not None and torch.isfinite(w.grad).all() and w.grad.abs().sum() > 0 for w in layer.parameters())
    opt.step()
    assert all(not torch.equal(w, b) for w, b in zip(layer.parameters(), before))


@pytest.mark.parametrize("heads", [1, 3])
def test_gatconv_under_the_mask(qgtc, heads):
    import torch

    from qgtc_ppopp22_amd import conv

    n, F_in, C, rate, seed = 333, 12, 9, 0.6, 1
    adj, rng = _graph(torch, qgtc, n, 22)
    X = _dev(torch, rng.standard_normal((n, F_in)).astype(np.float32))
    torch.manual_seed(0)
    layer = conv.GATConv(F_in, C, heads=heads, edge_drop=rate).cuda()
    plain = conv.GATConv(F_in, C, heads=heads).cuda()
    plain.load_state_dict(layer.state_dict())
    for a in (adj, adj.T):
        h = torch.mm(X, layer.W)
        outs = []
        for i in range(heads):
            hi = h[:, i * C:(i + 1) * C].contiguous()
            outs.append(qgtc.tiledAggregate(a, hi, attn=(torch.mv(hi, layer.a_dst[i]), torch.mv(hi, layer.a_src[i])), negative_slope=0.2,
                                            edge_drop=(rate, seed)))
        want = outs[0] if heads == 1 else torch.cat(outs, dim=1)
        got = layer(a, X, edge_seed=seed)
        assert _same(torch, got, want)
        assert not _same(torch, got, plain(a, X))
    layer.eval()
    assert _same(torch, layer(adj, X), plain(adj, X)) and _same(torch, layer(adj, X, edge_seed=seed), plain(adj, X))
    layer.train()
    before = [w.detach().clone() for w in layer.parameters()]
    opt = torch.optim.SGD(layer.parameters(), lr=1e-2)
    layer(adj, X, edge_seed=seed).square().mean().backward()
    assert all(w.grad is not None and torch.isfinite(w.grad).all() and w.grad.abs().sum() > 0 for w in layer.parameters())
    opt.step()
    assert all(not torch.equal(w, b) for w, b in zip(layer.parameters(), before))
