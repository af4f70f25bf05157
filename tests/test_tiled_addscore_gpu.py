"""The additive edge score of GATv2 on the device (include/qgtc_addscore.h; tiled.tiledEdgeAdditiveScores and its gradients,
tiled.tiledEdgeAdditiveAttention on adj and adj.T) against the exact model of tests/tiled_addscore_model.py. The order of the
operations is part of the contract, so every comparison is bit for bit (against the NumPy model a NaN equals a NaN); nothing is sampled
and no tolerance is used.

Graphs, views and reorder flags: those of tests/test_tiled_esoftmax_gpu.py (n in {1, 33, 129, 300} straddle the 32-row and 128-column
tile edges; at 300 a hub column, a full tile, an empty row and an empty column; 300 once more reordered). Head shapes:
tiled_heads_model.HEAD_SHAPES + SDDMM_MORE_SHAPES for the score (every lane mapping and register path), HEAD_SHAPES for the gradients
(every width class of both views). Slopes 0, 0.2 and 1. Inputs: normal draws with entries forced so that own + nbr is exactly +0,
exactly -0 and negative (test_tiled_addscore_model.force_kinks)."""
import numpy as np
import pytest

import test_tiled_esoftmax_gpu as eg
import tiled_addscore_model as am
import tiled_heads_model as hm
from test_tiled_addscore_model import force_kinks

pytestmark = pytest.mark.gpu

GRAPHS, VIEWS = eg.GRAPHS, eg.VIEWS
SLOPES = (0.0, 0.2, 1.0)
_torch, _dev, graph, view, same_bits, identical = eg._torch, eg._dev, eg.graph, eg.view, eg.same_bits, eg.assert_floats_identical


def _rng(*key):
    return np.random.default_rng(list(key))


def _operands(g, H, d, *key):
    """own, nbr [n, H d] with the forced entries, att [H, d] with both signs, g [nnz, H]"""
    rng = _rng(g.n, H, d, *key)
    own, nbr = rng.normal(size=(g.n, H * d)).astype(np.float32), rng.normal(size=(g.n, H * d)).astype(np.float32)
    own, nbr = force_kinks(g.s, g.d, g.n, own, nbr)
    return own, nbr, rng.normal(size=(H, d)).astype(np.float32), rng.normal(size=(g.nnz, H)).astype(np.float32)


def _score(tiled, g, transposed, own, nbr, att, slope, H):
    """the entry itself on this view: the row view's kernel with the operands swapped on the other"""
    return tiled._addscore(g.adj, nbr, own, att, slope, H) if transposed else tiled._addscore(g.adj, own, nbr, att, slope, H)


@pytest.mark.parametrize("transposed", VIEWS)
@pytest.mark.parametrize("n,reorder", GRAPHS)
def test_the_score_equals_the_model_and_the_single_head_call(n, reorder, transposed):
    _torch()
    from qgtc_ppopp22_amd import tiled

    g = graph(n, reorder)
    a = view(g, transposed)
    seen = set()
    for i, (H, d) in enumerate(hm.HEAD_SHAPES + hm.SDDMM_MORE_SHAPES):
        seen.add(hm.sddmm_heads_variant(H * d, H))
        on, nn, an, _ = _operands(g, H, d)
        own, nbr, att = _dev(on), _dev(nn), _dev(an)
        for slope in SLOPES:
            s = _score(tiled, g, transposed, own, nbr, att, slope, H)
            assert s.shape == (g.nnz, H) and s.is_contiguous()
            identical(s, am.addscore_heads_f32(g.s, g.d, n, on, nn, an, slope, H, transposed), f"the model, H={H} d={d} slope={slope}")
        slope = SLOPES[i % 3]
        s = _score(tiled, g, transposed, own, nbr, att, slope, H)
        for h in range(H):   # every head is the heads = 1 call on contiguous slices
            c = slice(h * d, (h + 1) * d)
            one = tiled.tiledEdgeAdditiveScores(a, own[:, c].contiguous(), nbr[:, c].contiguous(), att[h].contiguous(), slope)
            assert one.shape == (g.nnz,) and same_bits(s[:, h], one), f"head {h} of H={H} d={d}"
        pub = tiled.tiledEdgeAdditiveScores(a, own, nbr, att, slope, heads=H)
        assert pub.shape == ((g.nnz, H) if H > 1 else (g.nnz,)) and same_bits(pub.reshape(g.nnz, H), s)
        assert same_bits(tiled.tiledEdgeAdditiveScores(a, own, nbr, att.view(-1), slope, heads=H).reshape(g.nnz, H), s), "att as [N]"
        assert same_bits(_score(tiled, g, transposed, own, nbr, att, slope, H), s), "two launches"
    assert len(seen) == 7, "every lane mapping and register path"


@pytest.mark.parametrize("transposed", VIEWS)
@pytest.mark.parametrize("n,reorder", GRAPHS)
def test_the_gradient_folds_equal_the_model_and_the_single_head_call(n, reorder, transposed):
    _torch()
    from qgtc_ppopp22_amd import tiled

    g = graph(n, reorder)
    a = view(g, transposed)
    for i, (H, d) in enumerate(hm.HEAD_SHAPES):   # N = 5 .. 320: every width class of both views, and chunks of columns
        on, nn, an, gn = _operands(g, H, d, 1)
        own, nbr, att, gs = _dev(on), _dev(nn), _dev(an), _dev(gn)
        for slope in SLOPES:
            want_d, want_P = am.addscore_grad_heads_f32(g.s, g.d, n, on, nn, an, slope, gn, H, transposed)
            d_own, P = tiled._addscore_grad(a, own, nbr, att, slope, gs, H, True, True)
            identical(d_own, want_d, f"d_own, H={H} d={d} slope={slope}")
            identical(P, want_P, f"P, H={H} d={d} slope={slope}")
            # one output alone is the same fold (on the column view a wider kernel)
            assert same_bits(tiled._addscore_grad(a, own, nbr, att, slope, gs, H, True, False)[0], d_own), f"d_own alone, H={H} d={d}"
            assert same_bits(tiled._addscore_grad(a, own, nbr, att, slope, gs, H, False, True)[1], P), f"P alone, H={H} d={d}"
        slope = SLOPES[i % 3]
        d_own, P = tiled._addscore_grad(a, own, nbr, att, slope, gs, H, True, True)
        for h in range(H):
            c = slice(h * d, (h + 1) * d)
            d1, P1 = tiled._addscore_grad(a, own[:, c].contiguous(), nbr[:, c].contiguous(), att[h].contiguous(), slope,
                                          gs[:, h].contiguous(), 1, True, True)
            assert same_bits(d_own[:, c], d1) and same_bits(P[:, c], P1), f"head {h} of H={H} d={d}"
        d2, P2 = tiled._addscore_grad(a, own, nbr, att, slope, gs, H, True, True)
        assert same_bits(d2, d_own) and same_bits(P2, P), "two launches"


@pytest.mark.parametrize("transposed", VIEWS)
@pytest.mark.parametrize("n,reorder", GRAPHS)
def test_autograd_gives_the_models_gradients(n, reorder, transposed):
    torch = _torch()
    from qgtc_ppopp22_amd import tiled

    g = graph(n, reorder)
    a = view(g, transposed)
    for i, (H, d) in enumerate(hm.HEAD_SHAPES):
        slope = SLOPES[i % 3]
        on, nn, an, gn = _operands(g, H, d, 2)
        own, nbr, att = (_dev(t).requires_grad_(True) for t in (on, nn, an))
        s = tiled.tiledEdgeAdditiveScores(a, own, nbr, att, slope, heads=H)
        s.backward(_dev(gn).view(s.shape))
        want_d, want_P = am.addscore_grad_heads_f32(g.s, g.d, n, on, nn, an, slope, gn, H, transposed)
        want_nbr, _ = am.addscore_grad_heads_f32(g.s, g.d, n, nn, on, an, slope, gn, H, not transposed)
        identical(own.grad, want_d, f"own.grad, H={H} d={d}")
        identical(nbr.grad, want_nbr, f"nbr.grad, H={H} d={d}")
        assert att.grad.shape == (H, d) and same_bits(att.grad, _dev(want_P).sum(dim=0).view(H, d)), f"att.grad, H={H} d={d}"


@pytest.mark.parametrize("transposed", VIEWS)
@pytest.mark.parametrize("n,reorder", GRAPHS)
def test_the_composed_attention_equals_the_composition_of_the_models(n, reorder, transposed):
    _torch()
    from qgtc_ppopp22_amd import tiled

    g = graph(n, reorder)
    a = view(g, transposed)
    for i, (H, d) in enumerate(hm.HEAD_SHAPES):
        slope = SLOPES[i % 3]
        dv = (3, d)[i % 2]   # V's heads need not be as wide as the scores'
        on, nn, an, _ = _operands(g, H, d, 3)
        rng = _rng(n, H, d, 4)
        Vn, dYn = rng.normal(size=(n, H * dv)).astype(np.float32), rng.normal(size=(n, H * dv)).astype(np.float32)
        own, nbr, att, V = (_dev(t).requires_grad_(True) for t in (on, nn, an, Vn))
        Y = tiled.tiledEdgeAdditiveAttention(a, own, nbr, V, att, slope, heads=H)
        Y.backward(_dev(dYn))
        identical(Y, am.additive_attention_heads_f32(g.s, g.d, n, on, nn, Vn, an, slope, H, transposed)[0], f"the output, H={H} d={d}")
        w_own, w_nbr, w_V, w_P = am.additive_attention_grads_heads_f32(g.s, g.d, n, on, nn, Vn, an, slope, H, dYn, transposed)
        identical(own.grad, w_own, f"d own, H={H} d={d}")
        identical(nbr.grad, w_nbr, f"d nbr, H={H} d={d}")
        identical(V.grad, w_V, f"dV, H={H} d={d}")
        assert same_bits(att.grad, _dev(w_P).sum(dim=0).view(H, d)), f"d att, H={H} d={d}"


def test_a_gradient_not_required_is_not_launched(monkeypatch):
    torch = _torch()
    from qgtc_ppopp22_amd import tiled

    g = graph(33)
    H, d = 3, 5
    calls = []
    real = {name: getattr(tiled, name) for name in ("_addscore", "_addscore_grad", "_weighted", "_edge_softmax_grad", "_sddmm")}
    for name, fn in real.items():
        monkeypatch.setattr(tiled, name, lambda *a, _fn=fn, _name=name, **k: (calls.append((_name,) + tuple(a[7:9])), _fn(*a, **k))[1])
    on, nn, an, gn = _operands(g, H, d, 5)
    own, nbr, att, gs = _dev(on), _dev(nn), _dev(an), _dev(gn)

    def run(*leaves):
        calls.clear()
        ops = [t.clone().requires_grad_(True) if k in leaves else t for k, t in enumerate((own, nbr, att))]
        tiled.tiledEdgeAdditiveScores(g.adj, *ops, 0.2, heads=H).backward(gs)
        return calls[1:]

    assert run(0) == [("_addscore_grad", True, False)]                      # own alone: d_own on the view
    assert run(2) == [("_addscore_grad", False, True)]                      # att alone: P on the view
    assert run(0, 2) == [("_addscore_grad", True, True)]                    # both: still one launch
    assert run(1) == [("_addscore_grad", True, False)]                      # nbr alone: the other view only
    assert run(0, 1, 2) == [("_addscore_grad", True, True), ("_addscore_grad", True, False)]
    calls.clear()
    assert not tiled.tiledEdgeAdditiveScores(g.adj, own, nbr, att, 0.2, heads=H).requires_grad
    assert [c[0] for c in calls] == ["_addscore"]
    # the composed attention with every leaf: three launches forward, five backward
    calls.clear()
    leaves = [t.clone().requires_grad_(True) for t in (own, nbr, att)]
    V = own.clone().requires_grad_(True)
    tiled.tiledEdgeAdditiveAttention(g.adj, leaves[0], leaves[1], V, leaves[2], 0.2, heads=H).sum().backward()
    assert [c[0] for c in calls] == ["_addscore", "_weighted", "_weighted", "_sddmm", "_edge_softmax_grad", "_addscore_grad", "_addscore_grad"]
    # with V alone the score's backward does not run
    calls.clear()
    tiled.tiledEdgeAdditiveAttention(g.adj, own, nbr, own.clone().requires_grad_(True), att, 0.2, heads=H).sum().backward()
    assert [c[0] for c in calls] == ["_addscore", "_weighted", "_weighted"]
    # and there is no second derivative
    X = own.clone().requires_grad_(True)
    gx, = torch.autograd.grad(tiled.tiledEdgeAdditiveScores(g.adj, X, nbr, att, 0.2, heads=H), X, gs, create_graph=True)
    with pytest.raises(RuntimeError):
        gx.sum().backward()


@pytest.mark.parametrize("transposed", VIEWS)
def test_an_adjacency_without_cells_gives_zeros(transposed):
    torch = _torch()
    import QGTC
    from qgtc_ppopp22_amd import tiled

    from qgtc_ppopp22_amd import cabi

    # the entry itself without tiles: d_own and P, where given, are filled with +0 on the stream
    lib = cabi.load()
    entry = lib.qgtc_tiled_addscore_grad_heads_f32_t if transposed else lib.qgtc_tiled_addscore_grad_heads_f32
    x = _dev(np.ones((40, 6), dtype=np.float32))
    w = _dev(-np.ones(6, dtype=np.float32))
    idx = (None,) * (4 if transposed else 3)
    for give_d, give_P in ((True, True), (True, False), (False, True)):
        dd, PP = torch.ones_like(x), torch.ones_like(x)
        rc = entry(*idx, 0, 40, x.data_ptr(), x.data_ptr(), x.numel(), 6, w.data_ptr(), 6, 0.2, dd.data_ptr() if give_d else None,
                   PP.data_ptr() if give_P else None, x.numel(), None, None, None, 0, 2, None)
        assert rc == 0, lib.qgtc_strerror(rc).decode()
        torch.cuda.synchronize()
        assert (dd.view(torch.int32) == (0 if give_d else 0x3f800000)).all() and (PP.view(torch.int32) == (0 if give_P else 0x3f800000)).all()
    # the Python route on an adjacency whose only cell a doubled edge has unset
    e0, e1 = torch.tensor([0, 0], dtype=torch.int64, device="cuda"), torch.tensor([1, 1], dtype=torch.int64, device="cuda")
    adj = QGTC.pack_edges_tiled(e0, e1, 40)
    a = adj.T if transposed else adj
    assert tiled._value_index(adj)[2] == 0
    rng = _rng(40)
    own, nbr = (_dev(rng.normal(size=(40, 6)).astype(np.float32)).requires_grad_(True) for _ in range(2))
    att = _dev(-np.ones((2, 3), dtype=np.float32)).requires_grad_(True)
    s = tiled.tiledEdgeAdditiveScores(a, own, nbr, att, 0.2, heads=2)
    assert s.shape == (0, 2)
    s.sum().backward()
    for t in (own, nbr, att):
        assert (t.grad.view(torch.int32) == 0).all()   # +0, whatever att's sign


def test_refusals():
    torch = _torch()
    from qgtc_ppopp22_amd import tiled

    g = graph(129)
    rng = _rng(129, 7)
    X = _dev(rng.normal(size=(129, 12)).astype(np.float32))
    att = _dev(rng.normal(size=(3, 4)).astype(np.float32))
    for a in (g.adj, g.adj.T):
        for fn in (lambda *args, **kw: tiled.tiledEdgeAdditiveScores(a, *args, **kw),
                   lambda own, nbr, att, *r, **kw: tiled.tiledEdgeAdditiveAttention(a, own, nbr, X, att, *r, **kw)):
            assert fn(X, X, att, 0.2, heads=3).shape[0] in (g.nnz, 129)
            for bad in (X.double(), X.cpu().numpy(), X.half()):                       # dtype -> TypeError
                with pytest.raises(TypeError):
                    fn(bad, X, att, heads=3)
                with pytest.raises(TypeError):
                    fn(X, bad, att, heads=3)
            with pytest.raises(TypeError):
                fn(X, X, att.double(), heads=3)
            with pytest.raises(TypeError):
                fn(X, X, att, heads=3.0)
            for bad in (X[:-1], X[:, :6].contiguous(), X[:, :, None], X.cpu(), X.t().contiguous().t()):   # shape, device, stride
                with pytest.raises(ValueError):
                    fn(bad, X, att, heads=3)
                with pytest.raises(ValueError):
                    fn(X, bad, att, heads=3)
            for bad in (att[:2], att.view(4, 3), att.view(-1)[:11], att.cpu(), att.t().contiguous().t(), att[None]):
                with pytest.raises(ValueError):
                    fn(X, X, bad, heads=3)
            for slope in (-0.1, 1.5, float("nan")):
                with pytest.raises(ValueError, match="negative_slope"):
                    fn(X, X, att, slope, heads=3)
            for heads in (5, 0, -1, 24):
                with pytest.raises(ValueError, match="heads"):
                    fn(X, X, att.view(-1), heads=heads)
        with pytest.raises(ValueError, match="heads"):
            tiled.tiledEdgeAdditiveAttention(a, X, X, X[:, :10].contiguous(), att, heads=3)   # V's width
