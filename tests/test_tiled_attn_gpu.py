"""The attention tiled products on the device (QGTC.tiledMMFloat(attn=), QGTC.tiledAggregate(attn=), conv.GATConv and the C-ABI entries
behind them) against the exact model of tests/tiled_attn_model.py. Every operation of forward and backward is one float32 operation in
a fixed order, the exponential included, so every comparison is bit for bit: nothing is sampled and no tolerance is used."""
import ctypes

import numpy as np
import pytest

from stream_cases import Live, capture_and_replay, eager_results, empty, env_of, ordering_probe, warm_adjacency
from test_tiled_float_gpu import CANARY, NAN_WORD, NO_EDGES, assert_floats_identical
from tiled_attn_model import (ATT_FORWARD_VARIANTS, ATT_GRAD_VARIANTS, ATT_TRANSPOSED_VARIANTS, att_chunks, att_grad_variant, att_variant,
                              attention_f32, attention_grads_f32, lrelu_f32)
from tiled_float_model import neighbour_lists
from tiled_model import random_edges

pytestmark = pytest.mark.gpu

SWEEP_N = (1, 16, 17, 33, 65, 129, 257)
SWEEP_n = (97, 333, 1000)                          # n % 32 and n % 128 are nonzero
SWEEP = [(n, N) for N in SWEEP_N for n in SWEEP_n]


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _same(torch, a, b):
    return torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32))


def _inputs(rng, n, N, spread=1.0):
    X, dY = rng.standard_normal((n, N)).astype(np.float32), rng.standard_normal((n, N)).astype(np.float32)
    p, q = (rng.uniform(-1, 1, n) * spread).astype(np.float32), (rng.uniform(-1, 1, n) * spread).astype(np.float32)
    return X, dY, p, q


def _device_all(torch, qgtc, a, X, p, q, dY, slope):
    """(Y, m, inv, dX, dp, dq) from the public interface: tiledAggregate under autograd, tiledMMFloat for the statistics."""
    Xg, pg, qg = (_dev(torch, t).requires_grad_(True) for t in (X, p, q))
    Y = qgtc.tiledAggregate(a, Xg, attn=(pg, qg), negative_slope=slope)
    assert Y.requires_grad and Y.dtype == torch.float32 and Y.shape == X.shape and Y.is_contiguous()
    Y.backward(_dev(torch, dY))
    res = qgtc.tiledMMFloat(a, Xg.detach(), attn=(pg.detach(), qg.detach()), negative_slope=slope, return_stats=True)
    assert isinstance(res, tuple) and len(res) == 3
    out, m, inv = res
    assert m.shape == (a.n,) and inv.shape == (a.n,) and m.dtype == torch.float32 and inv.dtype == torch.float32
    assert _same(torch, out, Y)
    alone = qgtc.tiledMMFloat(a, Xg.detach(), attn=(pg.detach(), qg.detach()), negative_slope=slope)
    assert isinstance(alone, torch.Tensor) and _same(torch, alone, Y)
    return tuple(_np(t) for t in (Y, m, inv, Xg.grad, pg.grad, qg.grad))


def _model_all(src, dst, n, X, p, q, dY, slope, transposed):
    Y, m, inv = attention_f32(src, dst, n, X, p, q, slope, transposed)
    dX, dp, dq, _ = attention_grads_f32(src, dst, n, X, p, q, dY, Y, m, inv, slope, transposed)
    return Y, m, inv, dX, dp, dq


def _assert_all(got, want, what):
    for name, g, w in zip(("Y", "m", "inv", "dX", "dp", "dq"), got, want):
        assert_floats_identical(g, w, f"{what} {name}")


def _check_views(torch, qgtc, src, dst, n, X, p, q, dY, slope, what, adj=None, finite=True):
    adj = adj if adj is not None else qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    for transposed in (False, True):
        a = adj.T if transposed else adj
        want = _model_all(src, dst, n, X, p, q, dY, slope, transposed)
        if finite:
            assert all(np.isfinite(w).all() for w in want), what
        got = _device_all(torch, qgtc, a, X, p, q, dY, slope)
        _assert_all(got, want, f"{what} {'adj.T' if transposed else 'adj'} variant={att_variant(X.shape[1], transposed)}")
    return adj


# ---- 1. the sweep: every variant of both views and both modes, and of the score gradient ---------------------------------------------
def test_the_sweep_hits_every_variant():
    """Against tests/tiled_attn_model.py's copy of the launchers' switches (tiled_attn_kernels.hip.h, tiled_attn_t_kernels.hip.h). The
    backward
    mode of the product runs on the other view at the same N, so a sweep over both views covers both modes of both tables."""
    for transposed, variants in ((False, ATT_FORWARD_VARIANTS), (True, ATT_TRANSPOSED_VARIANTS)):
        assert sorted({att_variant(N, transposed) for N in SWEEP_N}) == sorted(variants)
        assert max(att_chunks(N, transposed) for N in SWEEP_N) >= 2
    assert sorted({att_grad_variant(N) for N in SWEEP_N}) == sorted(ATT_GRAD_VARIANTS)
    assert all(n % 32 and n % 128 for n in SWEEP_n)
    assert {n for n, _ in SWEEP} == set(SWEEP_n) and {N for _, N in SWEEP} == set(SWEEP_N) and len(SWEEP) == 21


@pytest.mark.parametrize("n,N", SWEEP, ids=[f"n{n}-N{N}" for n, N in SWEEP])
def test_every_variant_equals_the_model(qgtc, n, N):
    import torch

    rng = np.random.default_rng(17 * n + N)
    src, dst = random_edges(rng, n, 6 * n + 5)
    X, dY, p, q = _inputs(rng, n, N)
    _check_views(torch, qgtc, src, dst, n, X, p, q, dY, 0.2, f"n={n} N={N}")


# ---- 2. long lists ------------------------------------------------------------------------------------------------------------------------
def test_a_long_row_and_a_long_column(qgtc):
    """Hub h has 300 out-edges and 300 in-edges at n = 600: its row queues more than 32 neighbours (full queues are flushed), its
    k-quad's list has more than 8 tiles (several rounds of the column view)."""
    import torch

    n, h, N = 600, 301, 40
    rng = np.random.default_rng(4)
    others = rng.permutation(np.delete(np.arange(n, dtype=np.int64), h))[:300]
    extra = random_edges(rng, n, 2 * n)
    keep = (extra[0] != h) & (extra[1] != h)
    src = np.concatenate([np.full(300, h, np.int64), others, extra[0][keep]])
    dst = np.concatenate([others, np.full(300, h, np.int64), extra[1][keep]])
    X, dY, p, q = _inputs(rng, n, N, spread=3.0)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    t = adj.T
    assert int(adj.degrees()[h]) == 300 and int(t.degrees()[h]) == 300
    assert int((t.col_ptr[h // 128 + 1] - t.col_ptr[h // 128]).item()) > 8
    _check_views(torch, qgtc, src, dst, n, X, p, q, dY, 0.2, "hub", adj=adj)


# ---- 3. wide score spreads, masking, slopes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slope", [0.2, 1.0])
def test_score_spreads_beyond_the_exponential(qgtc, slope):
    """Scores up to +-200: many z fall below -87 and weigh exactly 0; nothing overflows and nothing is NaN."""
    import torch

    n, N = 333, 20
    rng = np.random.default_rng(9)
    src, dst = random_edges(rng, n, 8 * n)
    X, dY, p, q = _inputs(rng, n, N, spread=200.0)
    o, k, _ = neighbour_lists(src, dst, n)
    _, m, _ = attention_f32(src, dst, n, X, p, q, slope)
    with np.errstate(all="ignore"):
        assert ((lrelu_f32(p[o] + q[k], slope) - m[o]) < -87).sum() > n
    _check_views(torch, qgtc, src, dst, n, X, p, q, dY, slope, f"spread slope={slope}")


def _masked_scores(rng, src, dst, n, q, transposed):
    """q with about 40 % of the nodes at -inf, such that every row of the view keeps an unmasked neighbour; row r0's only unmasked
    neighbour is its last."""
    o, k, deg = neighbour_lists(src, dst, n, transposed)
    masked = rng.random(n) < 0.4
    r0 = int(np.flatnonzero((deg >= 6) & (deg <= 12))[0])
    first = k[o == r0]
    masked[first[:-1]], masked[first[-1]] = True, False
    for _ in range(n):
        alive = np.bincount(o[~masked[k]], minlength=n) > 0
        dead = np.flatnonzero((deg > 0) & ~alive)
        if not dead.size:
            break
        for r in dead:                             # unmask a neighbour r0 does not see, else the row's last
            mine = k[o == r]
            free = mine[~np.isin(mine, first[:-1])]
            masked[free[-1] if free.size else mine[-1]] = False
    assert masked[first[:-1]].all() and not masked[first[-1]], "row r0's only finite neighbour is its last"
    return np.where(masked, -np.inf, q).astype(np.float32), r0


def test_masked_neighbours(qgtc):
    import torch

    n, N = 333, 24
    rng = np.random.default_rng(12)
    src, dst = random_edges(rng, n, 5 * n)
    X, dY, p, q = _inputs(rng, n, N)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    for transposed in (False, True):
        qm, r0 = _masked_scores(rng, src, dst, n, q, transposed)
        assert np.isinf(qm).sum() > n // 5
        want = _model_all(src, dst, n, X, p, qm, dY, 0.2, transposed)
        assert all(np.isfinite(w).all() for w in want)
        got = _device_all(torch, qgtc, adj.T if transposed else adj, X, p, qm, dY, 0.2)
        _assert_all(got, want, f"masked transposed={transposed}")
        assert (got[5][np.isinf(qm)] == 0).all()                 # a masked neighbour takes part in nothing


@pytest.mark.parametrize("slope", [0.0, 0.2, 1.0])
def test_slopes(qgtc, slope):
    """Scores on a grid of eighths: e is exactly 0 on many edges, where the slope applies in the gradient."""
    import torch

    n, N = 333, 33
    rng = np.random.default_rng(21)
    src, dst = random_edges(rng, n, 6 * n + 5)
    X, dY, _, _ = _inputs(rng, n, N)
    p, q = (rng.integers(-8, 9, n) / 8).astype(np.float32), (rng.integers(-8, 9, n) / 8).astype(np.float32)
    o, k, _ = neighbour_lists(src, dst, n)
    assert ((p[o] + q[k]) == 0).sum() > 20
    _check_views(torch, qgtc, src, dst, n, X, p, q, dY, slope, f"slope={slope}")


# ---- 4. no edges, one node, a reordered adjacency -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,N,loop", [(1, 1, False), (1, 5, True), (300, 24, False), (97, 300, False)])
def test_an_empty_adjacency_and_one_node(qgtc, n, N, loop):
    import torch

    rng = np.random.default_rng(n + N)
    src, dst = (np.zeros(1, np.int64), np.zeros(1, np.int64)) if loop else NO_EDGES
    X, dY, p, q = _inputs(rng, n, N)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    assert adj.n_tiles == (1 if loop else 0)
    for transposed in (False, True):
        got = _device_all(torch, qgtc, adj.T if transposed else adj, X, p, q, dY, 0.2)
        _assert_all(got, _model_all(src, dst, n, X, p, q, dY, 0.2, transposed), f"n={n} loop={loop} transposed={transposed}")
        if loop:
            assert_floats_identical(got[0], X, "one self loop: the softmax of one logit is 1")
            assert got[2].tolist() == [1.0] and (got[4] == 0).all() and (got[5] == 0).all()
        else:
            assert all((g.view(np.uint32) == 0).all() for g in (got[0], got[2], got[3], got[4], got[5]))
            assert_floats_identical(got[1], lrelu_f32(p, 0.2), "m of a row without neighbours is L(p)")


def test_a_reordered_adjacency(qgtc):
    import torch

    n, N = 1000, 40
    rng = np.random.default_rng(31)
    src, dst = random_edges(rng, n, 6 * n + 5)
    X, dY, p, q = _inputs(rng, n, N)
    re = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n, reorder=True)
    rank = re.rank.cpu().numpy()
    assert (rank != np.arange(n)).any()
    _check_views(torch, qgtc, rank[src], rank[dst], n, X, p, q, dY, 0.2, "reordered", adj=re)
    # through to_new / to_old the edge list's numbering comes back: the same softmax, folded in another order
    Xo = _dev(torch, X)
    po, qo = _dev(torch, p), _dev(torch, q)
    got = re.to_old(qgtc.tiledMMFloat(re, re.to_new(Xo), attn=(re.to_new(po), re.to_new(qo))))
    want, _, _ = attention_f32(src, dst, n, X, p, q, 0.2)
    np.testing.assert_allclose(_np(got), want, rtol=0, atol=1e-5)


# ---- 5. autograd: subsets, strided dY, determinism ------------------------------------------------------------------------------------------
def test_needs_input_grad_subsets(qgtc):
    import torch

    n, N = 333, 70
    rng = np.random.default_rng(5)
    src, dst = random_edges(rng, n, 6 * n + 5)
    X, dY, p, q = _inputs(rng, n, N)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    for a in (adj, adj.T):
        full = _device_all(torch, qgtc, a, X, p, q, dY, 0.2)[3:]
        for mask in range(1, 8):
            ts = [_dev(torch, t).requires_grad_(bool(mask >> i & 1)) for i, t in enumerate((X, p, q))]
            qgtc.tiledAggregate(a, ts[0], attn=(ts[1], ts[2])).backward(_dev(torch, dY))
            for i, t in enumerate(ts):
                if mask >> i & 1:
                    assert_floats_identical(_np(t.grad), full[i], f"subset {mask:03b} gradient {i}")
                else:
                    assert t.grad is None
        ts = [_dev(torch, t) for t in (X, p, q)]
        assert not qgtc.tiledAggregate(a, ts[0], attn=(ts[1], ts[2])).requires_grad
    # a non-contiguous dY is made contiguous by the backward
    Xg = _dev(torch, X).requires_grad_(True)
    wide = _dev(torch, np.repeat(dY, 2, axis=1))
    qgtc.tiledAggregate(adj, Xg, attn=(_dev(torch, p), _dev(torch, q))).backward(wide[:, ::2])
    assert_floats_identical(_np(Xg.grad), _model_all(src, dst, n, X, p, q, dY, 0.2, False)[3], "strided dY")
    # no second derivative
    Xg = _dev(torch, X).requires_grad_(True)
    (g,) = torch.autograd.grad(qgtc.tiledAggregate(adj, Xg, attn=(_dev(torch, p), _dev(torch, q))).square().sum(), Xg, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()


def test_two_launches_give_identical_bits(qgtc):
    import torch

    n, N = 1000, 96
    rng = np.random.default_rng(6)
    src, dst = random_edges(rng, n, 6 * n + 5)
    X, dY, p, q = _inputs(rng, n, N, spread=4.0)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    for a in (adj, adj.T):
        first, again = (_device_all(torch, qgtc, a, X, p, q, dY, 0.2) for _ in range(2))
        for f, g in zip(first, again):
            assert (f.view(np.uint32) == g.view(np.uint32)).all(), a.transposed
        assert all(np.count_nonzero(f) > n // 2 for f in first)


# ---- 6. streams and graph capture -----------------------------------------------------------------------------------------------------------
def _live(env, transposed):
    """Forward and all three gradients as a ``Live`` case of tests/stream_cases.py; the reference is the eager result on the default
    stream."""
    torch = env.torch
    n, N = 600, 40
    rng = np.random.default_rng(41)
    src, dst = random_edges(rng, n, 6 * n + 5)
    adj = warm_adjacency(env, src, dst, n)
    a = adj.T if transposed else adj
    data = [_inputs(rng, n, N) for _ in range(4)]      # (X, dY, p, q)
    X, dY, p, q = bufs = [empty(env, t.shape, torch.float32) for t in data[0]]
    for t in (X, p, q):
        t.requires_grad_(True)

    def run():
        Y = env.Q.tiledAggregate(a, X, attn=(p, q))
        return [Y.detach(), *torch.autograd.grad(Y, (X, p, q), dY)]

    return Live(torch, bufs, data, eager_results(torch, bufs, data, run), run=run, keep=adj)


@pytest.mark.parametrize("transposed", [False, True], ids=["adj", "adjT"])
def test_side_stream_and_graph_capture(qgtc, oracle, transposed):
    """Forward and all three gradients behind a timed head start on three fresh side streams (``ordering_probe``) and captured into a
    graph; three replays on new inputs equal the eager results (``capture_and_replay``)."""
    import torch

    live = _live(env_of(qgtc, oracle, torch), transposed)
    what = f"attention, {'adj.T' if transposed else 'adj'}"
    ordering_probe(torch, qgtc, live, what)
    capture_and_replay(torch, qgtc, live, what)


# ---- 7. the C entries write what they own and nothing else --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,N", [(97, 17), (333, 129)])
def test_the_c_entries_stay_within_their_outputs(qgtc, n, N):
    import torch

    from qgtc_ppopp22_amd import cabi

    L = cabi.load()
    rng = np.random.default_rng(n)
    src, dst = random_edges(rng, n, 6 * n + 5)
    X, dY, p, q = _inputs(rng, n, N)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    dX_, ddY, dp_, dq_ = (_dev(torch, t) for t in (X, dY, p, q))
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fresh(elems):
        return torch.full((elems + CANARY,), float("nan"), dtype=torch.float32, device="cuda")

    def taken(buf, elems):
        a = buf.cpu().numpy()
        assert (a[elems:].view(np.uint32) == NAN_WORD).all(), "canaries"
        return a[:elems]

    for transposed in (False, True):
        t = adj.T
        idx = (t.col_ptr.data_ptr(), t.col_tile.data_ptr(), t.col_rb.data_ptr(), adj.tiles.data_ptr()) if transposed else \
            (adj.row_ptr.data_ptr(), adj.kquad.data_ptr(), adj.tiles.data_ptr())
        sfx = "_t" if transposed else ""
        Y, m, inv, gX, gp, gq = _model_all(src, dst, n, X, p, q, dY, 0.2, transposed)
        M = qgtc.tiledMMFloat(t if transposed else adj, dq_.unsqueeze(1), reduce="max").reshape(n)
        out, mo, io = fresh(n * N), fresh(n), fresh(n)
        rc = getattr(L, "qgtc_tiledatt_f32" + sfx)(*idx, adj.n_tiles, n, dX_.data_ptr(), n * N, N, dp_.data_ptr(), dq_.data_ptr(), 0.2, 0,
                                                   M.data_ptr(), mo.data_ptr(), io.data_ptr(), out.data_ptr(), n * N, st)
        assert rc == 0
        assert_floats_identical(taken(out, n * N).reshape(n, N), Y, "C forward")
        assert_floats_identical(taken(mo, n), m, "C m")
        assert_floats_identical(taken(io, n), inv, "C inv")
        dm, di, dYd = _dev(torch, m), _dev(torch, inv), _dev(torch, Y)
        D = fresh(n)
        assert L.qgtc_rowdot_f32(ddY.data_ptr(), dYd.data_ptr(), n * N, n, N, D.data_ptr(), n, st) == 0
        Dn = taken(D, n)
        assert_floats_identical(Dn, attention_grads_f32(src, dst, n, X, p, q, dY, Y, m, inv, 0.2, transposed)[3], "C row dot")
        g = fresh(n)
        rc = getattr(L, "qgtc_tiledatt_grad_f32" + sfx)(*idx, adj.n_tiles, n, ddY.data_ptr(), dX_.data_ptr(), n * N, N, dp_.data_ptr(),
                                                        dq_.data_ptr(), 0.2, 0, dm.data_ptr(), di.data_ptr(), D.data_ptr(), g.data_ptr(), n, st)
        assert rc == 0
        assert_floats_identical(taken(g, n), gp, "C dp")
        # the other two gradients of the forward on the OTHER view run on this one: its dX and dq
        Yo, m_o, inv_o, gXo, _, gqo = _model_all(src, dst, n, X, p, q, dY, 0.2, not transposed)
        dmo, dio = _dev(torch, m_o), _dev(torch, inv_o)
        out = fresh(n * N)
        rc = getattr(L, "qgtc_tiledatt_f32" + sfx)(*idx, adj.n_tiles, n, ddY.data_ptr(), n * N, N, dq_.data_ptr(), dp_.data_ptr(), 0.2, 1,
                                                   dmo.data_ptr(), None, dio.data_ptr(), out.data_ptr(), n * N, st)
        assert rc == 0
        assert_floats_identical(taken(out, n * N).reshape(n, N), gXo, "C dX")
        Do = _dev(torch, attention_grads_f32(src, dst, n, X, p, q, dY, Yo, m_o, inv_o, 0.2, not transposed)[3])
        g = fresh(n)
        rc = getattr(L, "qgtc_tiledatt_grad_f32" + sfx)(*idx, adj.n_tiles, n, dX_.data_ptr(), ddY.data_ptr(), n * N, N, dq_.data_ptr(),
                                                        dp_.data_ptr(), 0.2, 1, dmo.data_ptr(), dio.data_ptr(), Do.data_ptr(), g.data_ptr(), n, st)
        assert rc == 0
        assert_floats_identical(taken(g, n), gqo, "C dq")


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals(qgtc):
    import torch

    from qgtc_ppopp22_amd.conv import GATConv

    n, N = 100, 8
    src, dst = random_edges(np.random.default_rng(8), n, 6 * n)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    good = torch.ones(n, N, dtype=torch.float32, device="cuda")
    s = torch.ones(n, dtype=torch.float32, device="cuda")
    for a in (adj, adj.T):
        for fn in (qgtc.tiledMMFloat, qgtc.tiledAggregate):
            with pytest.raises(ValueError, match="row_scale"):
                fn(a, good, row_scale=s, attn=(s, s))
            with pytest.raises(ValueError, match="src_scale"):
                fn(a, good, src_scale=s, attn=(s, s))
            for name in ("max", "min"):
                with pytest.raises(ValueError, match="reduce"):
                    fn(a, good, reduce=name, attn=(s, s))
            for bad in (-0.1, 1.5, float("nan"), float("inf")):
                with pytest.raises(ValueError, match="negative_slope"):
                    fn(a, good, attn=(s, s), negative_slope=bad)
            # the scores follow the scales' rules, under their own names
            with pytest.raises(TypeError, match="att_out"):
                fn(a, good, attn=(s.double(), s))
            with pytest.raises(TypeError, match="att_nbr"):
                fn(a, good, attn=(s, [1.0] * n))
            with pytest.raises(ValueError, match="att_nbr"):
                fn(a, good, attn=(s, s[:-1]))
            with pytest.raises(ValueError, match="att_out"):
                fn(a, good, attn=(torch.ones(2 * n, device="cuda")[::2], s))
            with pytest.raises(ValueError, match="att_out"):
                fn(a, good, attn=(s.cpu(), s))
            with pytest.raises(TypeError, match="attn"):
                fn(a, good, attn=s)
            with pytest.raises(TypeError, match="attn"):
                fn(a, good, attn=(s, s, s))
            with pytest.raises(TypeError, match="float16"):
                fn(a, good.half(), attn=(s, s))
            with pytest.raises(ValueError, match="strides"):
                fn(a, torch.ones(N, n, dtype=torch.float32, device="cuda").t(), attn=(s, s))
        with pytest.raises(ValueError, match="return_arg"):
            qgtc.tiledMMFloat(a, good, attn=(s, s), return_arg=True)
        with pytest.raises(ValueError, match="return_stats"):
            qgtc.tiledMMFloat(a, good, return_stats=True)
        with pytest.raises(ValueError, match="return_stats"):
            qgtc.tiledMMFloat(a, good, reduce="max", return_stats=True)
    with pytest.raises(TypeError, match="TiledAdjacency"):
        qgtc.tiledAggregate((adj.row_ptr, adj.kquad, adj.tiles), good, attn=(s, s))
    # the binding's keyword overload
    from qgtc_ppopp22_amd.tiled import _ext

    with pytest.raises(RuntimeError, match="att_mode"):
        _ext._tiled_mm_f32(adj.row_ptr, adj.kquad, adj.tiles, n, good, att_mode="sideways", att_own=s, att_nbr=s, shift=s)
    with pytest.raises(RuntimeError, match="shift"):
        _ext._tiled_mm_f32(adj.row_ptr, adj.kquad, adj.tiles, n, good, att_mode="forward", att_own=s, att_nbr=s)
    with pytest.raises(RuntimeError, match="inv"):
        _ext._tiled_mm_f32(adj.row_ptr, adj.kquad, adj.tiles, n, good, att_mode="backward", att_own=s, att_nbr=s, shift=s)
    with pytest.raises(RuntimeError, match="negative_slope"):
        _ext._tiled_mm_f32(adj.row_ptr, adj.kquad, adj.tiles, n, good, att_mode="forward", att_own=s, att_nbr=s, shift=s, negative_slope=2.0)
    # without attn every call is the one it was
    assert torch.equal(qgtc.tiledMMFloat(adj, good, attn=None), qgtc.tiledMMFloat(adj, good))
    assert torch.equal(qgtc.tiledAggregate(adj, good, s, attn=None), qgtc.tiledMMFloat(adj, good, s))
    # the layer
    with pytest.raises(ValueError, match="heads"):
        GATConv(8, 8, heads=0)
    with pytest.raises(ValueError, match="negative_slope"):
        GATConv(8, 8, negative_slope=1.5)
    layer = GATConv(N, 4).cuda()
    with pytest.raises(NotImplementedError, match="TiledAdjacency"):
        layer(torch.zeros(n, n, device="cuda"), good)
    assert layer(adj, good).shape == (n, 4)


# ---- 9. the layer -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads,concat", [(1, True), (3, True), (3, False)])
def test_gatconv_equals_the_composition(qgtc, heads, concat):
    import torch

    from qgtc_ppopp22_amd.conv import GATConv

    n, F_in, F_out = 1213, 48, 20
    torch.manual_seed(0)
    src, dst = random_edges(np.random.default_rng(n), n, 8 * n)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n, reorder=True)
    assert adj.perm is not None
    X = torch.randn(n, F_in, device="cuda")
    target = torch.randint(0, F_out, (n,), device="cuda")
    layer = GATConv(F_in, F_out, heads=heads, negative_slope=0.1, concat=concat).cuda()
    assert layer.W.shape == (F_in, heads * F_out) and layer.a_dst.shape == (heads, F_out) and layer.a_src.shape == (heads, F_out)

    def composed(a, W, a_dst, a_src, agg):
        h = torch.mm(a.to_new(X), W)
        outs = []
        for i in range(heads):
            hi = h[:, i * F_out:(i + 1) * F_out].contiguous()
            outs.append(agg(a, hi, attn=(torch.mv(hi, a_dst[i]), torch.mv(hi, a_src[i])), negative_slope=0.1))
        if heads == 1:
            return a.to_old(outs[0])
        return a.to_old(torch.cat(outs, dim=1) if concat else torch.stack(outs).mean(dim=0))

    for a in (adj, adj.T):
        with torch.no_grad():
            want = composed(a, layer.W, layer.a_dst, layer.a_src, qgtc.tiledMMFloat)
            got = layer(a, X)
        assert got.shape == (n, heads * F_out if concat else F_out) and _same(torch, got, want), a.transposed
        assert torch.isfinite(got).all()
        # one SGD step: the gradients are those of the same composition built from tiledAggregate, and every parameter moves
        opt = torch.optim.SGD(layer.parameters(), lr=0.1)
        opt.zero_grad(set_to_none=True)
        out = layer(a, X)
        torch.nn.functional.cross_entropy(out[:, :F_out], target).backward()
        twins = [t.detach().clone().requires_grad_(True) for t in (layer.W, layer.a_dst, layer.a_src)]
        torch.nn.functional.cross_entropy(composed(a, *twins, qgtc.tiledAggregate)[:, :F_out], target).backward()
        before = [t.detach().clone() for t in (layer.W, layer.a_dst, layer.a_src)]
        for name, prm, twin in zip(("W", "a_dst", "a_src"), (layer.W, layer.a_dst, layer.a_src), twins):
            assert torch.isfinite(prm.grad).all() and prm.grad.abs().max() > 0, name
            assert _same(torch, prm.grad, twin.grad), name
        opt.step()
        for name, prm, old in zip(("W", "a_dst", "a_src"), (layer.W, layer.a_dst, layer.a_src), before):
            assert not torch.equal(prm.detach(), old), name
