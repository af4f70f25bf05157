"""The edge softmax of the tiled adjacency on the device (tiled.tiledEdgeSoftmax with its gradient, tiled.tiledEdgeScores,
tiled.tiledEdgeAttention on adj and adj.T) against the exact model of tests/tiled_esoftmax_model.py and against the attention launches.
The order of the operations is part of the contract, so every comparison is bit for bit (against the NumPy model a NaN equals a NaN);
nothing is sampled and no tolerance is used.

Graphs: those of tests/test_tiled_edge_gpu.py - n in {1, 33, 129, 300}; at n = 300 a hub column (its k-quad's column list exceeds a
round of staged tiles, its softmax folds 290 terms), a full tile (val_row reaches its largest values), a row and a column without
edges; n = 300 once more with reorder=True."""
import functools

import numpy as np
import pytest

import tiled_attn_model as am
import tiled_edge_model as em
import tiled_esoftmax_model as sm

pytestmark = pytest.mark.gpu

GRAPHS = [(n, False) for n in (1, 33, 129, 300)] + [(300, True)]
VIEWS = [False, True]


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    return torch


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def assert_floats_identical(got, want, what=""):
    """Bit for bit (so -0.0 is not 0.0), except that any NaN equals any NaN."""
    if hasattr(got, "detach"):
        got = got.detach().cpu().numpy()
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    np.testing.assert_array_equal(gn, wn, err_msg=f"{what}: NaN positions")
    np.testing.assert_array_equal(got.view(np.uint32)[~gn], want.view(np.uint32)[~wn], err_msg=what)


def same_bits(a, b):
    import torch

    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class Graph:
    """One test graph: the adjacency, and the edge list in the adjacency's numbering (`s`, `d`, NumPy) that the model works on."""

    def __init__(self, n, reorder):
        _torch()
        import QGTC

        src, dst = sm.graph_edges(n)
        self.n = n
        self.adj = QGTC.pack_edges_tiled(_dev(src), _dev(dst), n, reorder=reorder)
        if reorder:
            rank = self.adj.rank.cpu().numpy()
            self.s, self.d = rank[src], rank[dst]
        else:
            self.s, self.d = src, dst
        self.row, self.col = em.slot_cells(self.s, self.d, n)
        self.nnz = self.row.size
        rng = np.random.default_rng(7 * n + 1)
        self.logits = (3 * rng.normal(size=self.nnz)).astype(np.float32)
        self.g = rng.normal(size=self.nnz).astype(np.float32)


@functools.lru_cache(maxsize=None)
def graph(n, reorder=False):
    return Graph(n, reorder)


def view(g, transposed):
    return g.adj.T if transposed else g.adj


@pytest.mark.parametrize("transposed", VIEWS)
@pytest.mark.parametrize("n,reorder", GRAPHS)
def test_forward_statistics_and_gradient_equal_the_model(n, reorder, transposed):
    torch = _torch()
    from qgtc_ppopp22_amd import tiled

    g = graph(n, reorder)
    a = view(g, transposed)
    alpha, m, inv = tiled.tiledEdgeSoftmax(a, _dev(g.logits), return_stats=True)
    wa, wm, wi = sm.edge_softmax_f32(g.s, g.d, n, g.logits, transposed)
    assert alpha.shape == (g.nnz,) and m.shape == (n,) and inv.shape == (n,)
    assert_floats_identical(alpha, wa, "alpha")
    assert_floats_identical(m, wm, "m")
    assert_floats_identical(inv, wi, "inv")
    assert same_bits(tiled.tiledEdgeSoftmax(a, _dev(g.logits)), alpha), "without the statistics: the same weights"
    # the gradient, through autograd and on a vector of its own
    L = _dev(g.logits).requires_grad_(True)
    tiled.tiledEdgeSoftmax(a, L).backward(_dev(g.g))
    want = sm.edge_softmax_grad_f32(g.s, g.d, n, wa, g.g, transposed)
    assert_floats_identical(L.grad, want, "dlogits")
    # two launches give the same bits
    a2, m2, i2 = tiled.tiledEdgeSoftmax(a, _dev(g.logits), return_stats=True)
    assert same_bits(a2, alpha) and same_bits(m2, m) and same_bits(i2, inv)
    L2 = _dev(g.logits).requires_grad_(True)
    tiled.tiledEdgeSoftmax(a, L2).backward(_dev(g.g))
    assert same_bits(L2.grad, L.grad)
    # a gradient that is not required is not launched, and there is no second derivative
    assert not tiled.tiledEdgeSoftmax(a, _dev(g.logits)).requires_grad
    if g.nnz:
        L3 = _dev(g.logits).requires_grad_(True)
        gl, = torch.autograd.grad(tiled.tiledEdgeSoftmax(a, L3), L3, _dev(g.g), create_graph=True)
        with pytest.raises(RuntimeError):
            gl.sum().backward()


@pytest.mark.parametrize("transposed", VIEWS)
@pytest.mark.parametrize("n,reorder", [(129, False), (300, False), (300, True)])
def test_minus_infinity_masks_an_edge_and_owners_without_cells(n, reorder, transposed):
    _torch()
    from qgtc_ppopp22_amd import tiled

    g = graph(n, reorder)
    a = view(g, transposed)
    owner, _, slot, deg = sm.owner_lists(g.s, g.d, n, transposed)
    start = np.concatenate([[0], np.cumsum(deg)[:-1]])
    big, big3 = np.flatnonzero(deg >= 2), np.flatnonzero(deg >= 3)
    # the first cell of every owner with two or more, the last one too where there are three or more: every owner keeps a finite logit
    masked = np.concatenate([slot[start[big]], slot[start[big3] + deg[big3] - 1]])
    l2 = g.logits.copy()
    l2[masked] = -np.inf
    alpha, m, inv = tiled.tiledEdgeSoftmax(a, _dev(l2), return_stats=True)
    wa, wm, wi = sm.edge_softmax_f32(g.s, g.d, n, l2, transposed)
    assert_floats_identical(alpha, wa)
    assert_floats_identical(m, wm)
    assert_floats_identical(inv, wi)
    got = alpha.cpu().numpy()
    assert (got[masked].view(np.uint32) == 0).all(), "a masked edge weighs +0"
    assert np.isfinite(got).all()
    none = deg == 0
    assert none.any(), "the graph has an owner without cells on either view"
    assert (m.cpu().numpy()[none].view(np.uint32) == 0).all() and (inv.cpu().numpy()[none].view(np.uint32) == 0).all()
    # the gradient of the masked softmax: +-0 at the masked edges, the model's bits everywhere
    L = _dev(l2).requires_grad_(True)
    tiled.tiledEdgeSoftmax(a, L).backward(_dev(g.g))
    assert_floats_identical(L.grad, sm.edge_softmax_grad_f32(g.s, g.d, n, wa, g.g, transposed))
    assert (L.grad.cpu().numpy()[masked] == 0).all()


@pytest.mark.parametrize("transposed", VIEWS)
def test_a_nan_logit_stays_with_its_owner(transposed):
    _torch()
    from qgtc_ppopp22_amd import tiled

    g = graph(300)
    a = view(g, transposed)
    owner, _, slot, deg = sm.owner_lists(g.s, g.d, g.n, transposed)
    owner_of_slot = np.zeros(g.nnz, dtype=np.int64)
    owner_of_slot[slot] = owner
    bad_owner = int(np.flatnonzero(deg >= 3)[2])
    l2 = g.logits.copy()
    l2[slot[np.flatnonzero(owner == bad_owner)[1]]] = np.nan
    alpha, m, inv = tiled.tiledEdgeSoftmax(a, _dev(l2), return_stats=True)
    wa, wm, wi = sm.edge_softmax_f32(g.s, g.d, g.n, g.logits, transposed)
    others = owner_of_slot != bad_owner
    assert_floats_identical(alpha.cpu().numpy()[others], wa[others])
    keep = np.arange(g.n) != bad_owner
    assert_floats_identical(m.cpu().numpy()[keep], wm[keep])
    assert_floats_identical(inv.cpu().numpy()[keep], wi[keep])


@pytest.mark.parametrize("transposed", VIEWS)
@pytest.mark.parametrize("n,reorder", GRAPHS)
def test_statistics_equal_the_attention_launch(n, reorder, transposed):
    torch = _torch()
    import QGTC
    from qgtc_ppopp22_amd import tiled

    g = graph(n, reorder)
    a = view(g, transposed)
    rng = np.random.default_rng(n + 11)
    p, q = _dev(rng.normal(size=n).astype(np.float32)), _dev(rng.normal(size=n).astype(np.float32))
    X = _dev(rng.normal(size=(n, 3)).astype(np.float32))
    row, col = tiled.edge_endpoints(g.adj)
    own, nbr = (col, row) if transposed else (row, col)
    e = p[own.long()] + q[nbr.long()]
    logits = torch.where(e > 0, e, 0.2 * e)
    assert_floats_identical(logits, sm.pair_logits(g.s, g.d, n, p.cpu().numpy(), q.cpu().numpy(), 0.2, transposed), "the logits in torch")
    _, m, inv = tiled.tiledEdgeSoftmax(a, logits, return_stats=True)
    _, m_att, inv_att = QGTC.tiledMMFloat(a, X, attn=(p, q), return_stats=True)
    assert same_bits(inv, inv_att)
    has = a.degrees() > 0
    assert same_bits(m[has], m_att[has])


@pytest.mark.parametrize("d", [16, 300])
@pytest.mark.parametrize("transposed", VIEWS)
@pytest.mark.parametrize("n,reorder", GRAPHS)
def test_scores_and_attention_equal_the_model_composed(n, reorder, transposed, d):
    torch = _torch()
    from qgtc_ppopp22_amd import tiled

    assert {em.sddmm_variant(16), em.sddmm_variant(300)} == set(em.SDDMM_VARIANTS)
    g = graph(n, reorder)
    a = view(g, transposed)
    rng = np.random.default_rng(1000 * n + d)
    N = 7
    Qn, Kn = rng.normal(size=(n, d)).astype(np.float32), rng.normal(size=(n, d)).astype(np.float32)
    Vn, dYn = rng.normal(size=(n, N)).astype(np.float32), rng.normal(size=(n, N)).astype(np.float32)
    # the scores and their two gradients
    Q, K = _dev(Qn).requires_grad_(True), _dev(Kn).requires_grad_(True)
    s = tiled.tiledEdgeScores(a, Q, K)
    assert_floats_identical(s, em.sddmm_f32(g.s, g.d, n, Qn, Kn, transposed), "scores")
    s.backward(_dev(g.g))
    assert_floats_identical(Q.grad, em.weighted_f32(g.s, g.d, n, Kn, g.g, transposed), "dA")
    assert_floats_identical(K.grad, em.weighted_f32(g.s, g.d, n, Qn, g.g, not transposed), "dB")
    # the attention, with the default scale and with one given
    for scale in (None, 0.37):
        sc = 1.0 / np.sqrt(d) if scale is None else scale
        Q, K, V = (_dev(t).requires_grad_(True) for t in (Qn, Kn, Vn))
        Y = tiled.tiledEdgeAttention(a, Q, K, V, scale=scale)
        want, _, _ = sm.edge_attention_f32(g.s, g.d, n, Qn, Kn, Vn, sc, transposed)
        assert_floats_identical(Y, want, f"attention, scale {scale}")
        Y.backward(_dev(dYn))
        for got, w, what in zip((Q.grad, K.grad, V.grad), sm.edge_attention_grads_f32(g.s, g.d, n, Qn, Kn, Vn, sc, dYn, transposed),
                                ("dQ", "dK", "dV")):
            assert_floats_identical(got, w, f"{what}, scale {scale}")
    # each gradient alone
    Q, K, V = _dev(Qn), _dev(Kn), _dev(Vn).requires_grad_(True)
    tiled.tiledEdgeAttention(a, Q, K, V, scale=0.37).backward(_dev(dYn))
    assert Q.grad is None and K.grad is None
    assert_floats_identical(V.grad, sm.edge_attention_grads_f32(g.s, g.d, n, Qn, Kn, Vn, 0.37, dYn, transposed)[2], "dV alone")


def test_a_gradient_not_required_is_not_launched(monkeypatch):
    _torch()
    from qgtc_ppopp22_amd import tiled

    g = graph(33)
    calls = []
    real_mm, real_grad = tiled.tiledMMFloat, tiled._edge_softmax_grad
    monkeypatch.setattr(tiled, "tiledMMFloat", lambda *a, **k: (calls.append("mm"), real_mm(*a, **k))[1])
    monkeypatch.setattr(tiled, "_edge_softmax_grad", lambda *a, **k: (calls.append("grad"), real_grad(*a, **k))[1])
    rng = np.random.default_rng(3)
    A, B = _dev(rng.normal(size=(33, 5)).astype(np.float32)), _dev(rng.normal(size=(33, 5)).astype(np.float32))
    tiled.tiledEdgeScores(g.adj, A.clone().requires_grad_(True), B).backward(_dev(g.g))
    assert calls == ["mm"]
    calls.clear()
    tiled.tiledEdgeScores(g.adj, A, B.clone().requires_grad_(True)).backward(_dev(g.g))
    assert calls == ["mm"]
    calls.clear()
    L = _dev(g.logits).requires_grad_(True)
    tiled.tiledEdgeSoftmax(g.adj, L).backward(_dev(g.g))
    assert calls == ["grad"]


def test_refusals():
    torch = _torch()
    from qgtc_ppopp22_amd import tiled

    g = graph(129)
    adj, L = g.adj, _dev(g.logits)
    for a in (adj, adj.T):
        with pytest.raises(ValueError):
            tiled.tiledEdgeSoftmax(a, L[:-1])                         # a wrong length
        with pytest.raises(ValueError):
            tiled.tiledEdgeSoftmax(a, L[:, None])
        with pytest.raises(TypeError):
            tiled.tiledEdgeSoftmax(a, L.double())                     # a wrong dtype
        with pytest.raises(TypeError):
            tiled.tiledEdgeSoftmax(a, g.logits)                       # not a tensor
        with pytest.raises(ValueError):
            tiled.tiledEdgeSoftmax(a, L.cpu())                        # a wrong device
        with pytest.raises(ValueError):
            tiled.tiledEdgeSoftmax(a, torch.stack([L, L], 1)[:, 0])   # not contiguous
    with pytest.raises(TypeError):
        tiled.tiledEdgeSoftmax(None, L)
    X = torch.zeros((g.n, 4), device="cuda")
    with pytest.raises(ValueError):
        tiled.tiledEdgeScores(adj, X, X[:, :2].contiguous())
    with pytest.raises(TypeError):
        tiled.tiledEdgeScores(adj, X.double(), X.double())
    with pytest.raises(ValueError):
        tiled.tiledEdgeAttention(adj, X, X, X[:-1])
    for name in ("tiledEdgeSoftmax", "tiledEdgeScores", "tiledEdgeAttention"):
        assert name in tiled.__all__
