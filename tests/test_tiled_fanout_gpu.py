"""Fixed-fanout sampling on the device (``fanout=`` of QGTC.tiledMMFloat / QGTC.tiledAggregate, qgtc_ppopp22_amd.fanout and the C entries
of include/qgtc_fanout.h) against tests/tiled_fanout_model.py: the selection launches give the model's thresholds word for word on both
axes, and masking is dropping, so every sampled operator must give, bit for bit, what the exact models give on the kept edges and what
the unmasked operator gives on ``pack_edges_tiled`` of the kept edges - in the own form (a sample taken on the view used) and in the nbr
form (a sample taken on the other view). No tolerance anywhere."""
import numpy as np
import pytest

import tiled_drop_model as dm
import tiled_fanout_model as fm
from test_tiled_drop_gpu import NAMES, _assert_all, _dev, _forwards, _grads, _inputs, _models, _np, _same
from test_tiled_float_gpu import NO_EDGES, assert_floats_identical
from tiled_attn_model import (ATT_FORWARD_VARIANTS, ATT_GRAD_VARIANTS, ATT_TRANSPOSED_VARIANTS, att_grad_variant, att_variant,
                              attention_grads_f32)
from tiled_float_model import FLOAT_FORWARD_VARIANTS, FLOAT_TRANSPOSED_VARIANTS, float_variant, neighbour_lists
from tiled_max_model import MAX_FORWARD_VARIANTS, MAX_TRANSPOSED_VARIANTS, max_variant
from tiled_model import random_edges

pytestmark = pytest.mark.gpu

SWEEP_N = (1, 16, 17, 33, 65, 129, 257)
SWEEP_n = (97, 333, 1000)                          # n % 32 and n % 128 are nonzero
KS = (1, 3, 8)
# the grid N x n x k x seed, thinned as tests/test_tiled_drop_gpu.py thins its own: every (n, N) runs both views and both forms under one
# k and one seed, which rotate
SWEEP = [(n, N, KS[(iN + i) % 3], dm.SEEDS[(2 * iN + i) % 4]) for iN, N in enumerate(SWEEP_N) for i, n in enumerate(SWEEP_n)]


def _fanout():
    from qgtc_ppopp22_amd import fanout

    return fanout


def _thr(sample):
    return sample.thr.cpu().numpy().view(np.uint32)


def _pack(torch, qgtc, src, dst, n):
    return qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)


# ---- 1. the thresholds ------------------------------------------------------------------------------------------------------------------
def _assert_thresholds(torch, qgtc, src, dst, n, ks, seeds, what):
    adj = _pack(torch, qgtc, src, dst, n)
    for k in ks:
        for seed in seeds:
            for axis, view in (("row", adj), ("col", adj.T)):
                got = _thr(_fanout().sample_fanout(view, k, seed))
                np.testing.assert_array_equal(got, fm.thresholds(src, dst, n, k, seed, axis), err_msg=f"{what} k={k} seed={seed:#x} {axis}")
    return adj


@pytest.mark.parametrize("n", [1, 97, 333, 1000])
def test_thresholds_equal_the_model(qgtc, n):
    import torch

    rng = np.random.default_rng(7 * n)
    src, dst = random_edges(rng, n, 6 * n + 5)
    _assert_thresholds(torch, qgtc, src, dst, n, (1, 2, 5, 32, n), (dm.SEEDS[n % 4], dm.SEEDS[(n + 1) % 4]), f"n={n}")


def test_thresholds_without_edges(qgtc):
    import torch

    for n in (1, 300):
        adj = _assert_thresholds(torch, qgtc, *NO_EDGES, n, (1, 4), (1,), f"no edges n={n}")
        assert (_thr(_fanout().sample_fanout(adj, 2, 5)) == 0).all()


def test_thresholds_at_degree_k_and_k_plus_one(qgtc):
    """Row r has exactly r % 9 out-neighbours, column c exactly ... in-neighbours of its own pattern: with k = 4 the degrees k - 1, k and
    k + 1 all occur; degree k gives 0, degree k + 1 the second smallest hash."""
    import torch

    n, k = 200, 4
    rows = np.repeat(np.arange(n), np.arange(n) % 9)
    cols = (rows * 7 + np.concatenate([np.arange(d) for d in np.arange(n) % 9]) * 13) % n
    for src, dst, axis in ((rows, cols, "row"), (cols, rows, "col")):
        _, _, deg = neighbour_lists(src, dst, n, axis == "col")
        assert {k - 1, k, k + 1} <= set(deg.tolist())
        adj = _assert_thresholds(torch, qgtc, src, dst, n, (k,), (1, 2 ** 64 - 1), "degree k")
        thr = _thr(_fanout().sample_fanout(adj.T if axis == "col" else adj, k, 1))
        assert (thr[deg <= k] == 0).all() and (thr[deg > k] != 0).all()


def test_thresholds_at_the_tile_edges(qgtc):
    """Cells at columns 127 / 128 (two k-quads, the last bit of one word row and the first of the next) and rows 31 / 32 (two row blocks),
    in rows and columns dense enough to be sampled."""
    import torch

    n = 300
    rng = np.random.default_rng(3)
    hot = np.array([31, 32, 127, 128])
    other = np.arange(n)
    src = np.concatenate([np.repeat(hot, n), np.tile(other, 4), rng.integers(0, n, 500)])
    dst = np.concatenate([np.tile(other, 4), np.repeat(hot, n), rng.integers(0, n, 500)])
    _assert_thresholds(torch, qgtc, src, dst, n, (1, 2, 127, 128, 299), (0, 0x0123456789ABCDEF), "tile edges")


def test_thresholds_of_the_complete_graph(qgtc):
    import torch

    n = 200
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    _assert_thresholds(torch, qgtc, i.ravel(), j.ravel(), n, (7,), (1,), "complete")


def test_thresholds_of_a_hub(qgtc):
    """n = 5000 with one full row and one full column: 157 tiles in the hub's row block and 157 entries in its k-quad's list, more hashes
    than a wave holds in LDS, so the selection walks the tiles once per bit. k = 1, 64 and n - 1."""
    import torch

    n, h = 5000, 2345
    rng = np.random.default_rng(9)
    extra = random_edges(rng, n, 2 * n)
    allv = np.arange(n)
    src = np.concatenate([np.full(n, h), allv, extra[0]])
    dst = np.concatenate([allv, np.full(n, h), extra[1]])
    adj = _assert_thresholds(torch, qgtc, src, dst, n, (1, 64, 4999), (1,), "hub")
    for view, axis in ((adj, "row"), (adj.T, "col")):
        thr = _thr(_fanout().sample_fanout(view, 64, 1))
        hashes = dm.H(h, allv, 1) if axis == "row" else dm.H(allv, h, 1)
        assert thr[h] == np.sort(hashes)[n - 64] and int((hashes >= thr[h]).sum()) == 64


# ---- 2. the aggregates ------------------------------------------------------------------------------------------------------------------
def test_the_sweep_reaches_every_launcher_variant():
    """Against the models' copies of the launchers' switches: the _fanout entries go through their parents' launchers (one per kernel
    family), so they choose as their parents do. Every case runs the plain sum, each scale alone and both, max and min, the attention
    forward and its three gradients on both views, each in both forms."""
    for transposed, fl, mx, at in ((False, FLOAT_FORWARD_VARIANTS, MAX_FORWARD_VARIANTS, ATT_FORWARD_VARIANTS),
                                   (True, FLOAT_TRANSPOSED_VARIANTS, MAX_TRANSPOSED_VARIANTS, ATT_TRANSPOSED_VARIANTS)):
        assert sorted({float_variant(N, transposed) for N in SWEEP_N}) == sorted(fl)
        assert sorted({max_variant(N, transposed) for N in SWEEP_N}) == sorted(mx)
        assert sorted({att_variant(N, transposed) for N in SWEEP_N}) == sorted(at)
    assert sorted({att_grad_variant(N) for N in SWEEP_N}) == sorted(ATT_GRAD_VARIANTS)
    assert len(SWEEP) == 21 and {s[0] for s in SWEEP} == set(SWEEP_n) and {s[1] for s in SWEEP} == set(SWEEP_N)
    assert {s[2] for s in SWEEP} == set(KS) and {s[3] for s in SWEEP} == set(dm.SEEDS)
    for k in KS:                                   # every k meets every n and at least five widths
        assert {s[0] for s in SWEEP if s[2] == k} == set(SWEEP_n)
        assert len({s[1] for s in SWEEP if s[2] == k}) >= 5
    for N in SWEEP_N:                              # every width runs under all three k
        assert {s[2] for s in SWEEP if s[1] == N} == set(KS)


def _check(torch, qgtc, src, dst, n, N, k, seed, rng, what, adj=None, repack=True):
    """both axes x both views: the sampled operators on `adj` against the models on the kept edges and, with `repack`, against the
    unmasked operators on the adjacency packed from the kept edges. The sample is passed as (k, seed) in the own form once, and as a
    FanoutSample everywhere else."""
    X, dY, p, q, r, c = _inputs(rng, n, N)
    adj = adj if adj is not None else _pack(torch, qgtc, src, dst, n)
    for axis, taken_on in (("row", adj), ("col", adj.T)):
        ks, kd = fm.kept_edges(src, dst, n, k, seed, axis)
        kadj = _pack(torch, qgtc, ks, kd, n) if repack else None
        sample = _fanout().sample_fanout(taken_on, k, seed)
        for transposed in (False, True):
            a = adj.T if transposed else adj
            form = "own" if a is taken_on else "nbr"
            w = f"{what} axis={axis} {'adj.T' if transposed else 'adj'} ({form}) k={k} seed={seed:#x}"
            got = _forwards(torch, qgtc, a, X, p, q, r, c, fanout=sample)
            _assert_all(got, _models(ks, kd, n, X, p, q, r, c, transposed), w + " against the model")
            if form == "own":
                _assert_all(_forwards(torch, qgtc, a, X, p, q, r, c, fanout=(k, seed)), got, w + " as a pair")
            if repack:
                _assert_all(got, _forwards(torch, qgtc, kadj.T if transposed else kadj, X, p, q, r, c), w + " against the re-packed adjacency")
            Y, m, inv = got[8:]
            want = attention_grads_f32(ks, kd, n, X, p, q, dY, Y, m, inv, 0.2, transposed)[:3]
            for name, g, wv in zip(("dX", "dp", "dq"), _grads(torch, qgtc, a, X, dY, p, q, r, c, "attn", fanout=sample)[1:], want):
                assert_floats_identical(g, wv, f"{w} attention {name}")
    return adj, (X, dY, p, q, r, c)


@pytest.mark.parametrize("n,N,k,seed", SWEEP, ids=[f"n{n}-N{N}-k{k}-s{dm.SEEDS.index(s)}" for n, N, k, s in SWEEP])
def test_sampled_operators_equal_the_model_and_the_repacked_adjacency(qgtc, n, N, k, seed):
    import torch

    rng = np.random.default_rng(17 * n + N)
    src, dst = random_edges(rng, n, 6 * n + 5)
    _check(torch, qgtc, src, dst, n, N, k, seed, rng, f"n={n} N={N}")


def test_a_hub_keeps_more_than_a_queue(qgtc):
    """Hub h has 300 out-edges and 300 in-edges at n = 600; k = 40 keeps more than the 32 ids a queue holds, with dropped neighbours in
    between, and on the other view the hub is a neighbour of 300 rows of which 40 keep it."""
    import torch

    n, h, N, k, seed = 600, 301, 40, 40, 1
    rng = np.random.default_rng(4)
    others = rng.permutation(np.delete(np.arange(n, dtype=np.int64), h))[:300]
    extra = random_edges(rng, n, 2 * n)
    keep = (extra[0] != h) & (extra[1] != h)
    src = np.concatenate([np.full(300, h, np.int64), others, extra[0][keep]])
    dst = np.concatenate([others, np.full(300, h, np.int64), extra[1][keep]])
    _check(torch, qgtc, src, dst, n, N, k, seed, rng, "hub")


@pytest.mark.parametrize("n,N,loop", [(1, 1, False), (1, 5, True), (300, 24, False)])
def test_an_empty_adjacency_and_one_node(qgtc, n, N, loop):
    import torch

    rng = np.random.default_rng(n + N)
    src, dst = (np.zeros(1, np.int64), np.zeros(1, np.int64)) if loop else NO_EDGES
    _check(torch, qgtc, src, dst, n, N, 1, 1, rng, f"n={n} loop={loop}")


def test_a_reordered_adjacency(qgtc):
    """The sample is in the adjacency's own numbering: the model hashes the NEW ids."""
    import torch

    n, N, k, seed = 1000, 40, 3, 2 ** 64 - 1
    rng = np.random.default_rng(31)
    src, dst = random_edges(rng, n, 6 * n + 5)
    re = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n, reorder=True)
    rank = re.rank.cpu().numpy()
    _check(torch, qgtc, rank[src], rank[dst], n, N, k, seed, rng, "reordered", adj=re, repack=False)


def test_a_fanout_of_the_largest_degree_is_the_plain_call(qgtc):
    import torch

    n, N = 333, 70
    rng = np.random.default_rng(2)
    src, dst = random_edges(rng, n, 6 * n + 5)
    X, dY, p, q, r, c = _inputs(rng, n, N)
    adj = _pack(torch, qgtc, src, dst, n)
    for a in (adj, adj.T):
        plain = _forwards(torch, qgtc, a, X, p, q, r, c)
        d = int(a.degrees().max())
        assert not np.array_equal(_forwards(torch, qgtc, a, X, p, q, r, c, fanout=(d - 1, 1))[0].view(np.uint32), plain[0].view(np.uint32))
        for k in (d, d + 1, n, 2 ** 31 - 1, 2 ** 40):
            for seed in dm.SEEDS[:2]:
                _assert_all(_forwards(torch, qgtc, a, X, p, q, r, c, fanout=(k, seed)), plain, f"k={k} seed {seed:#x}")
                sample = _fanout().sample_fanout(a, k, seed)
                assert (_thr(sample) == 0).all()
                _assert_all(_forwards(torch, qgtc, a.T, X, p, q, r, c, fanout=sample), _forwards(torch, qgtc, a.T, X, p, q, r, c), "nbr form")
        _assert_all(_forwards(torch, qgtc, a, X, p, q, r, c, fanout=None), plain, "fanout=None")


# ---- 3. tiledAggregate -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["sym", "max", "attn"])
def test_backward_equals_the_unmasked_composition_on_the_repacked_adjacency(qgtc, mode, monkeypatch):
    """The gradients of X (and of p and q for the attention) equal those on the re-packed kept adjacency, with (k, seed) and with a
    sample of either view; a forward plus backward with (k, seed) issues ONE selection launch, with a sample none."""
    import torch

    n, N, k, seed = 333, 70, 3, 1
    rng = np.random.default_rng(5)
    src, dst = random_edges(rng, n, 6 * n + 5)
    X, dY, p, q, r, c = _inputs(rng, n, N)
    adj = _pack(torch, qgtc, src, dst, n)
    fo = _fanout()
    launches = []
    real = fo.sample_fanout
    counted = lambda *a, **kw: (launches.append(a[1:]), real(*a, **kw))[1]
    monkeypatch.setattr(fo, "sample_fanout", counted)
    monkeypatch.setattr(fo.tiled, "sample_fanout", counted)   # where fanout=(k, seed) of the aggregates draws: fanout re-exports it
    subsets = [(bool(m & 1), bool(m & 2), bool(m & 4)) for m in range(1, 8)] if mode == "attn" else [(True, False, False)]
    for transposed in (False, True):
        a = adj.T if transposed else adj
        ks, kd = fm.kept_edges(src, dst, n, k, seed, "col" if transposed else "row")
        kadj = _pack(torch, qgtc, ks, kd, n)
        ka = kadj.T if transposed else kadj
        other_view_sample = real(a, k, seed)       # taken on `a`: own on `a`, and what the pair draws
        for needs in subsets:
            del launches[:]
            got = _grads(torch, qgtc, a, X, dY, p, q, r, c, mode, needs, fanout=(k, seed))
            assert launches == [(k, seed)], "one selection launch in the forward, none in the backward"
            del launches[:]
            again = _grads(torch, qgtc, a, X, dY, p, q, r, c, mode, needs, fanout=other_view_sample)
            assert launches == []
            want = _grads(torch, qgtc, ka, X, dY, p, q, r, c, mode, needs)
            plain = _grads(torch, qgtc, a, X, dY, p, q, r, c, mode, needs)
            for i, (g, g2, w, u) in enumerate(zip(got, again, want, plain)):
                assert (g is None) == (w is None) and (g is None) == (i > 0 and not needs[i - 1]), (needs, i)
                if g is not None:
                    assert_floats_identical(g, w, f"{mode} {needs} output {i} transposed={transposed}")
                    assert_floats_identical(g2, w, f"{mode} {needs} output {i} transposed={transposed} from a sample")
                    assert (g.view(np.uint32) != u.view(np.uint32)).any(), "the sample changes the result"
        # a sample of the OTHER view: the forward runs in the nbr form and the backward in the own form
        ks2, kd2 = fm.kept_edges(src, dst, n, k, seed, "row" if transposed else "col")
        k2 = _pack(torch, qgtc, ks2, kd2, n)
        got = _grads(torch, qgtc, a, X, dY, p, q, r, c, mode, fanout=real(a.T, k, seed))
        want = _grads(torch, qgtc, k2.T if transposed else k2, X, dY, p, q, r, c, mode)
        for i, (g, w) in enumerate(zip(got, want)):
            if w is not None:
                assert_floats_identical(g, w, f"{mode} output {i} transposed={transposed} nbr-form forward")
    assert not qgtc.tiledAggregate(adj, _dev(torch, X), fanout=(k, seed)).requires_grad


def test_two_launches_agree_and_seeds_and_fanouts_differ(qgtc):
    import torch

    n, N = 1000, 96
    rng = np.random.default_rng(6)
    src, dst = random_edges(rng, n, 6 * n + 5)
    X, dY, p, q, r, c = _inputs(rng, n, N)
    adj = _pack(torch, qgtc, src, dst, n)
    for a in (adj, adj.T):
        first, again, other, wider = (_forwards(torch, qgtc, a, X, p, q, r, c, fanout=f) for f in ((3, 1), (3, 1), (3, 1 + 2 ** 32), (4, 1)))
        for name, f, g, o, w in zip(NAMES, first, again, other, wider):
            assert (f.view(np.uint32) == g.view(np.uint32)).all(), name
            assert (f.view(np.uint32) != o.view(np.uint32)).any(), name
            assert (f.view(np.uint32) != w.view(np.uint32)).any(), name
        s = _fanout().sample_fanout(a, 3, 1)
        assert s.view is a and s.k == 3 and s.seed == 1 and s.thr.dtype == torch.int32 and tuple(s.thr.shape) == (n,)
        kept = _np(qgtc.tiledMMFloat(a, torch.ones((n, 1), device="cuda"), fanout=s)).reshape(n)
        np.testing.assert_array_equal(kept, np.minimum(_np(a.degrees()), 3))   # exactly min(deg, k) per node, on the device


# ---- 4. SAGEConv -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aggr", ["mean", "max"])
def test_sageconv_equals_the_composition_of_the_public_operators(qgtc, aggr):
    import torch

    from qgtc_ppopp22_amd import sage

    n, F_in, C, k, seed = 333, 12, 9, 3, 0x0123456789ABCDEF
    rng = np.random.default_rng(21)
    src, dst = random_edges(rng, n, 6 * n + 5)
    adj = _pack(torch, qgtc, src, dst, n)
    X = _dev(torch, rng.standard_normal((n, F_in)).astype(np.float32))
    torch.manual_seed(0)
    layer = sage.SAGEConv(F_in, C, aggr=aggr, fanout=k).cuda()
    plain = sage.SAGEConv(F_in, C, aggr=aggr).cuda()
    plain.load_state_dict(layer.state_dict())
    for a in (adj, adj.T):
        deg = _np(a.degrees())
        scale = _dev(torch, np.where(deg > 0, np.float32(1) / np.minimum(np.maximum(deg, 1), k).astype(np.float32), np.float32(0)).astype(np.float32))
        assert _same(torch, layer.sampled_mean_scale(a), scale)          # 1 / min(deg, k), correctly rounded
        if aggr == "mean":
            agg = qgtc.tiledAggregate(a, X, scale, fanout=(k, seed))
        else:
            agg = qgtc.tiledAggregate(a, X, reduce="max", fanout=(k, seed))
        want = layer.lin_self(X) + layer.lin_nbr(agg)
        got = layer(a, X, seed=seed)
        assert _same(torch, got, want)
        assert not _same(torch, got, layer(a, X, seed=seed + 1)) and not _same(torch, got, plain(a, X))
        # a drawn seed follows torch's CPU generator
        torch.manual_seed(5)
        drawn = layer(a, X)
        torch.manual_seed(5)
        hi, lo = torch.randint(0, 1 << 32, (2,), dtype=torch.int64).tolist()
        assert _same(torch, drawn, layer(a, X, seed=(hi << 32) | lo))
        assert not _same(torch, drawn, layer(a, X))
    # eval: no sampling, the layer without the keyword bit for bit
    layer.eval()
    assert _same(torch, layer(adj, X), plain(adj, X)) and _same(torch, layer(adj, X, seed=seed), plain(adj, X))
    # one SGD step
    layer.train()
    before = [w.detach().clone() for w in layer.parameters()]
    opt = torch.optim.SGD(layer.parameters(), lr=1e-2)
    layer(adj, X, seed=seed).square().mean().backward()
    assert all(w.grad is not None and torch.isfinite(w.grad).all() and w.grad.abs().sum() > 0 for w in layer.parameters())
    opt.step()
    assert all(not torch.equal(w, b) for w, b in zip(layer.parameters(), before))


@pytest.mark.parametrize("aggr", ["mean", "max"])
def test_sageconv_against_a_dense_float64_definition(qgtc, aggr):
    """Forward, the gradient for X and every parameter gradient against the dense definition on the kept edges - the 0/1 matrix of
    tests/tiled_fanout_model.py's kept cells, a mean (or a masked maximum) over its rows - differentiated by torch.autograd in float64.
    The tolerance is the one tests/test_layers_dense_gpu.py uses, layers_reference.tolerances: tol(T) = 8 . max(max|T_f32 - T_f64|,
    2^-24 . max|T_f64|), computed from the dense definition alone in both precisions."""
    import torch

    import layers_reference as R
    from qgtc_ppopp22_amd import sage

    n, F_in, C, k, seed = 333, 12, 9, 3, 1
    rng = np.random.default_rng(23)
    src, dst = random_edges(rng, n, 6 * n + 5)
    adj = _pack(torch, qgtc, src, dst, n)
    X = rng.standard_normal((n, F_in)).astype(np.float32)
    dY = rng.standard_normal((n, C)).astype(np.float32)
    torch.manual_seed(0)
    layer = sage.SAGEConv(F_in, C, aggr=aggr, fanout=k).cuda()
    names = ("Y", "dX", "lin_self.weight", "lin_self.bias", "lin_nbr.weight")

    def dense(dtype, transposed):
        ks, kd = fm.kept_edges(src, dst, n, k, seed, "col" if transposed else "row")
        A = torch.zeros((n, n), dtype=torch.bool)
        A[torch.from_numpy(kd if transposed else ks), torch.from_numpy(ks if transposed else kd)] = True
        x = torch.from_numpy(X).to(dtype).requires_grad_(True)
        w = {name: t.detach().cpu().to(dtype).requires_grad_(True) for name, t in layer.named_parameters()}
        if aggr == "mean":
            deg = A.sum(dim=1).to(dtype)
            agg = (A.to(dtype) @ x) * torch.where(deg > 0, 1 / deg.clamp(min=1), torch.zeros((), dtype=dtype))[:, None]
        else:
            masked = torch.where(A[:, :, None], x[None, :, :], torch.full((), -float("inf"), dtype=dtype))
            agg = torch.where(A.any(dim=1)[:, None], masked.max(dim=1).values, torch.zeros((), dtype=dtype))
        Y = x @ w["lin_self.weight"].t() + w["lin_self.bias"] + agg @ w["lin_nbr.weight"].t()
        Y.backward(torch.from_numpy(dY).to(dtype))
        return dict(zip(names, (Y.detach(), x.grad, w["lin_self.weight"].grad, w["lin_self.bias"].grad, w["lin_nbr.weight"].grad)))

    for transposed in (False, True):
        a = adj.T if transposed else adj
        want, want32 = dense(torch.float64, transposed), dense(torch.float32, transposed)
        tol = R.tolerances(want, want32)
        layer.zero_grad()
        Xg = _dev(torch, X).requires_grad_(True)
        Y = layer(a, Xg, seed=seed)
        Y.backward(_dev(torch, dY))
        got = dict(zip(names, (Y, Xg.grad, layer.lin_self.weight.grad, layer.lin_self.bias.grad, layer.lin_nbr.weight.grad)))
        for name in names:
            err = float((got[name].detach().cpu().to(torch.float64) - want[name]).abs().max())
            print(f"transposed={transposed} {aggr} {name}: error / tolerance = {err / tol[name]:.3f} (tol {tol[name]:.3e})")
            assert tol[name] > 0 and err <= tol[name], (name, transposed)


def test_a_hand_built_sample_is_checked_before_any_launch(qgtc):
    """The C entries take no length for thr and the kernels index it by node id, so the Python layer refuses a tensor that is not the
    int32 [n] contiguous tensor on the adjacency's device - on both views, in either form."""
    import torch

    n = 97
    rng = np.random.default_rng(11)
    adj = _pack(torch, qgtc, *random_edges(rng, n, 4 * n), n)
    X = torch.zeros((n, 4), device="cuda")
    fo = _fanout()
    good = fo.sample_fanout(adj, 3, 1)
    for view in (adj, adj.T):
        for a in (adj, adj.T):
            for bad, error, match in ((good.thr.cpu(), ValueError, "device"), (good.thr[:-1], ValueError, "shape"),
                                      (good.thr.to(torch.int64), TypeError, "int32"),
                                      (torch.zeros(2 * n, dtype=torch.int32, device="cuda")[::2], ValueError, "contiguous")):
                with pytest.raises(error, match=match):
                    qgtc.tiledMMFloat(a, X, fanout=fo.FanoutSample(view, 3, 1, bad))
                with pytest.raises(error, match=match):
                    qgtc.tiledAggregate(a, X, reduce="max", fanout=fo.FanoutSample(view, 3, 1, bad))
    # a rebuilt sample with the same tensor is the sample
    again = fo.FanoutSample(adj, 3, 1, good.thr)
    for a in (adj, adj.T):
        assert _same(torch, qgtc.tiledMMFloat(a, X + 1, fanout=again), qgtc.tiledMMFloat(a, X + 1, fanout=good))
