"""All heads of the edge-value path in one launch (include/qgtc_heads.h; tiled.tiledSDDMM / tiledEdgeScores / tiledEdgeSoftmax /
tiledMMFloat / tiledAggregate / tiledEdgeAttention with heads, conv.TransformerConv) on the device. The contract is that every head is
bit for bit what the single-head call gives on the head's contiguous slice, so every comparison here is bit for bit: against the
existing single-head calls on `.contiguous()` slices and against the per-head models of tests/tiled_heads_model.py (against NumPy a
NaN equals a NaN). Nothing is sampled and no tolerance is used.

Graphs, views and reorder flags: those of tests/test_tiled_esoftmax_gpu.py (n in {1, 33, 129, 300} straddle the 32-row and 128-column
tile edges; at 300 a hub column, a full tile, an empty row and an empty column; 300 once more reordered). Head shapes:
tiled_heads_model.HEAD_SHAPES, which reach every lane mapping and register path of the per-edge dot, every width class of the weighted
sum and 1, 2 and 4 heads a lane in the softmax."""
import numpy as np
import pytest

import test_tiled_esoftmax_gpu as eg
import tiled_edge_model as em
import tiled_esoftmax_model as sm
import tiled_heads_model as hm

pytestmark = pytest.mark.gpu

GRAPHS, VIEWS = eg.GRAPHS, eg.VIEWS
assert (1, False) in GRAPHS
_torch, _dev, graph, view, same_bits, identical = eg._torch, eg._dev, eg.graph, eg.view, eg.same_bits, eg.assert_floats_identical


def _rng(*key):
    return np.random.default_rng(list(key))


def _col(t, h):
    """element [:, h] of a per-edge vector as a contiguous vector"""
    return t[:, h].contiguous()


def _heads_of(t, H, d):
    """the heads' column slices of a node matrix, contiguous"""
    return [t[:, h * d:(h + 1) * d].contiguous() for h in range(H)]


@pytest.mark.parametrize("transposed", VIEWS)
@pytest.mark.parametrize("n,reorder", GRAPHS)
def test_the_per_edge_dot_equals_the_single_head_call_and_the_model(n, reorder, transposed):
    _torch()
    from qgtc_ppopp22_amd import tiled

    g = graph(n, reorder)
    a = view(g, transposed)
    seen = set()
    for H, d in hm.HEAD_SHAPES + hm.SDDMM_MORE_SHAPES:
        seen.add(hm.sddmm_heads_variant(H * d, H))
        rng = _rng(n, H, d)
        An, Bn = rng.normal(size=(n, H * d)).astype(np.float32), rng.normal(size=(n, H * d)).astype(np.float32)
        A, B = _dev(An), _dev(Bn)
        # the entry itself, heads = 1 included (there it launches the single-head kernel)
        s = tiled._sddmm(g.adj, B, A, H) if transposed else tiled._sddmm(g.adj, A, B, H)
        assert s.shape == (g.nnz, H) and s.is_contiguous()
        identical(s, hm.sddmm_heads_f32(g.s, g.d, n, An, Bn, H, transposed), f"the model, H={H} d={d}")
        for h, (Ah, Bh) in enumerate(zip(_heads_of(A, H, d), _heads_of(B, H, d))):
            assert same_bits(_col(s, h), tiled.tiledSDDMM(a, Ah, Bh)), f"head {h} of H={H} d={d}"
        pub = tiled.tiledSDDMM(a, A, B, heads=H)
        assert pub.shape == ((g.nnz, H) if H > 1 else (g.nnz,)) and same_bits(pub.reshape(g.nnz, H), s)
        assert same_bits(tiled._sddmm(g.adj, B, A, H) if transposed else tiled._sddmm(g.adj, A, B, H), s), "two launches"
    assert len(seen) == 7, "every lane mapping and register path"


@pytest.mark.parametrize("transposed", VIEWS)
@pytest.mark.parametrize("n,reorder", GRAPHS)
def test_the_softmax_and_its_gradient_equal_the_single_head_call_and_the_model(n, reorder, transposed):
    _torch()
    from qgtc_ppopp22_amd import tiled

    g = graph(n, reorder)
    a = view(g, transposed)
    for H in sorted({H for H, _ in hm.HEAD_SHAPES}):   # 1, 2, 3, 4, 5, 8, 40: one, two and four heads a lane, several grid rows
        rng = _rng(n, H, 1)
        ln = (3 * rng.normal(size=(g.nnz, H))).astype(np.float32)
        gn = rng.normal(size=(g.nnz, H)).astype(np.float32)
        alpha, m, inv = tiled._edge_softmax(a, _dev(ln))
        assert alpha.shape == (g.nnz, H) and m.shape == (n, H) and inv.shape == (n, H)
        wa, wm, wi = hm.edge_softmax_heads_f32(g.s, g.d, n, ln, transposed)
        identical(alpha, wa, f"alpha, H={H}")
        identical(m, wm, f"m, H={H}")
        identical(inv, wi, f"inv, H={H}")
        dl = tiled._edge_softmax_grad(a, alpha, _dev(gn))
        identical(dl, hm.edge_softmax_grad_heads_f32(g.s, g.d, n, wa, gn, transposed), f"dlogits, H={H}")
        for h in range(H):
            a1, m1, i1 = tiled.tiledEdgeSoftmax(a, _dev(ln[:, h]), return_stats=True)
            assert same_bits(_col(alpha, h), a1) and same_bits(_col(m, h), m1) and same_bits(_col(inv, h), i1), f"head {h} of {H}"
            assert same_bits(_col(dl, h), tiled._edge_softmax_grad(a, a1, _dev(gn[:, h]))), f"gradient, head {h} of {H}"
        if H > 1:   # the public call and autograd
            L = _dev(ln).requires_grad_(True)
            pa, pm, pi = tiled.tiledEdgeSoftmax(a, L, return_stats=True)
            assert same_bits(pa, alpha) and same_bits(pm, m) and same_bits(pi, inv)
            pa.backward(_dev(gn))
            assert same_bits(L.grad, dl)


@pytest.mark.parametrize("transposed", VIEWS)
@pytest.mark.parametrize("n,reorder", GRAPHS)
def test_the_weighted_sum_equals_the_single_head_call_and_the_model(n, reorder, transposed):
    _torch()
    import QGTC
    from qgtc_ppopp22_amd import tiled

    g = graph(n, reorder)
    a = view(g, transposed)
    for H, d in hm.HEAD_SHAPES:   # N = 5 .. 320: every width class of both views, and chunks of columns
        rng = _rng(n, H, d, 2)
        Xn = rng.normal(size=(n, H * d)).astype(np.float32)
        vn = rng.normal(size=(g.nnz, H)).astype(np.float32)
        rn = rng.uniform(0.5, 2.0, size=n).astype(np.float32)
        X, v, r = _dev(Xn), _dev(vn), _dev(rn)
        for scale, sn in ((None, None), (r, rn)):
            Y = tiled._weighted(a, X, scale, v)
            identical(Y, hm.weighted_heads_f32(g.s, g.d, n, Xn, vn, transposed, sn), f"the model, H={H} d={d}")
            for h, Xh in enumerate(_heads_of(X, H, d)):
                assert same_bits(Y[:, h * d:(h + 1) * d], QGTC.tiledMMFloat(a, Xh, scale, edge_weight=_col(v, h))), f"head {h}, H={H} d={d}"
            if H > 1:
                assert same_bits(QGTC.tiledMMFloat(a, X, scale, edge_weight=v), Y)
        if H > 1:   # both gradients through autograd: the weights' is the per-edge dot with heads, X's the sum on the other view
            dYn = rng.normal(size=(n, H * d)).astype(np.float32)
            Xg, vg = _dev(Xn).requires_grad_(True), _dev(vn).requires_grad_(True)
            QGTC.tiledAggregate(a, Xg, r, edge_weight=vg).backward(_dev(dYn))
            sdY = (rn[:, None] * dYn).astype(np.float32)
            identical(Xg.grad, hm.weighted_heads_f32(g.s, g.d, n, sdY, vn, not transposed), f"dX, H={H} d={d}")
            identical(vg.grad, hm.sddmm_heads_f32(g.s, g.d, n, sdY, Xn, H, transposed), f"dvalues, H={H} d={d}")


@pytest.mark.parametrize("transposed", VIEWS)
@pytest.mark.parametrize("n,reorder", GRAPHS)
def test_attention_with_heads_equals_the_per_head_loop(n, reorder, transposed):
    torch = _torch()
    from qgtc_ppopp22_amd import tiled

    g = graph(n, reorder)
    a = view(g, transposed)
    for i, (H, d) in enumerate(hm.HEAD_SHAPES):
        rng = _rng(n, H, d, 3)
        dv = (3, d)[i % 2]   # V's heads need not be as wide as Q's
        Qn, Kn = rng.normal(size=(n, H * d)).astype(np.float32), rng.normal(size=(n, H * d)).astype(np.float32)
        Vn, dYn = rng.normal(size=(n, H * dv)).astype(np.float32), rng.normal(size=(n, H * dv)).astype(np.float32)
        for scale in (None, 0.37):
            Q, K, V = (_dev(t).requires_grad_(True) for t in (Qn, Kn, Vn))
            Y = tiled.tiledEdgeAttention(a, Q, K, V, scale=scale, heads=H)
            Y.backward(_dev(dYn))
            # the loop over the heads: today's single-head path on contiguous slices
            leaves = [[_dev(np.ascontiguousarray(t[:, h * w:(h + 1) * w])).requires_grad_(True) for h in range(H)]
                      for t, w in ((Qn, d), (Kn, d), (Vn, dv))]
            outs = [tiled.tiledEdgeAttention(a, leaves[0][h], leaves[1][h], leaves[2][h], scale=scale) for h in range(H)]
            torch.cat(outs, dim=1).backward(_dev(dYn))
            assert same_bits(Y, torch.cat(outs, dim=1)), f"output, H={H} d={d} scale={scale}"
            for got, per_head, what in zip((Q.grad, K.grad, V.grad), leaves, ("dQ", "dK", "dV")):
                assert same_bits(got, torch.cat([t.grad for t in per_head], dim=1)), f"{what}, H={H} d={d} scale={scale}"
        if n <= 129 or H <= 8:   # and the model, composed per head (the default scale is 1 / sqrt(d))
            identical(Y, hm.edge_attention_heads_f32(g.s, g.d, n, Qn, Kn, Vn, H, 0.37, transposed), f"the model, H={H} d={d}")
            for got, w, what in zip((Q.grad, K.grad, V.grad),
                                    hm.edge_attention_grads_heads_f32(g.s, g.d, n, Qn, Kn, Vn, H, dYn, 0.37, transposed), ("dQ", "dK", "dV")):
                identical(got, w, f"{what} of the model, H={H} d={d}")


@pytest.mark.parametrize("H", [3, 8])
@pytest.mark.parametrize("transposed", VIEWS)
def test_special_logits_stay_with_their_head(transposed, H):
    _torch()
    from qgtc_ppopp22_amd import tiled

    g = graph(300)
    a = view(g, transposed)
    owner, _, slot, deg = sm.owner_lists(g.s, g.d, g.n, transposed)
    start = np.concatenate([[0], np.cumsum(deg)[:-1]])
    owner_of_slot = np.zeros(g.nnz, dtype=np.int64)
    owner_of_slot[slot] = owner
    rng = _rng(300, H, 4)
    ln = (3 * rng.normal(size=(g.nnz, H))).astype(np.float32)
    clean = tiled._edge_softmax(a, _dev(ln))
    # -inf in head 1 only: the first cell of every owner with two or more, the last one too where there are three or more
    big, big3 = np.flatnonzero(deg >= 2), np.flatnonzero(deg >= 3)
    masked = np.concatenate([slot[start[big]], slot[start[big3] + deg[big3] - 1]])
    l2 = ln.copy()
    l2[masked, 1] = -np.inf
    alpha, m, inv = tiled.tiledEdgeSoftmax(a, _dev(l2), return_stats=True)
    for got, want in zip((alpha, m, inv), hm.edge_softmax_heads_f32(g.s, g.d, g.n, l2, transposed)):
        identical(got, want)
    got = alpha.cpu().numpy()
    assert (got[masked, 1].view(np.uint32) == 0).all() and np.isfinite(got).all(), "a masked edge weighs +0 in its head"
    others = [h for h in range(H) if h != 1]
    for t, c in zip((alpha, m, inv), clean):
        assert same_bits(t[:, others], c[:, others]), "the other heads do not see the mask"
    L = _dev(l2).requires_grad_(True)
    gn = rng.normal(size=(g.nnz, H)).astype(np.float32)
    tiled.tiledEdgeSoftmax(a, L).backward(_dev(gn))
    identical(L.grad, hm.edge_softmax_grad_heads_f32(g.s, g.d, g.n, got, gn, transposed))
    assert (L.grad.cpu().numpy()[masked, 1] == 0).all()
    # an owner without cells: +0 and (+0, 0) in every head
    none = deg == 0
    assert none.any(), "the graph has an owner without cells on either view"
    assert (m.cpu().numpy()[none].view(np.uint32) == 0).all() and (inv.cpu().numpy()[none].view(np.uint32) == 0).all()
    # a NaN in head H - 1 stays with its (owner, head)
    bad_owner, bad_head = int(np.flatnonzero(deg >= 3)[2]), H - 1
    l3 = ln.copy()
    l3[slot[np.flatnonzero(owner == bad_owner)[1]], bad_head] = np.nan
    na, nm, ni = tiled.tiledEdgeSoftmax(a, _dev(l3), return_stats=True)
    keep_slot = np.ones((g.nnz, H), dtype=bool)
    keep_slot[owner_of_slot == bad_owner, bad_head] = False
    keep_node = np.ones((g.n, H), dtype=bool)
    keep_node[bad_owner, bad_head] = False
    identical(na.cpu().numpy()[keep_slot], clean[0].cpu().numpy()[keep_slot])
    identical(nm.cpu().numpy()[keep_node], clean[1].cpu().numpy()[keep_node])
    identical(ni.cpu().numpy()[keep_node], clean[2].cpu().numpy()[keep_node])


def test_a_gradient_not_required_is_not_launched(monkeypatch):
    _torch()
    from qgtc_ppopp22_amd import tiled

    g = graph(33)
    H, d = 3, 5
    calls = []
    real = {name: getattr(tiled, name) for name in ("_weighted", "_edge_softmax_grad", "_sddmm")}
    for name, fn in real.items():
        monkeypatch.setattr(tiled, name, lambda *a, _fn=fn, _name=name, **k: (calls.append(_name), _fn(*a, **k))[1])
    rng = _rng(33, 5)
    A, B = _dev(rng.normal(size=(33, H * d)).astype(np.float32)), _dev(rng.normal(size=(33, H * d)).astype(np.float32))
    gs = _dev(rng.normal(size=(g.nnz, H)).astype(np.float32))
    tiled.tiledEdgeScores(g.adj, A.clone().requires_grad_(True), B, heads=H).backward(gs)
    assert calls == ["_sddmm", "_weighted"]
    calls.clear()
    tiled.tiledEdgeScores(g.adj, A, B.clone().requires_grad_(True), heads=H).backward(gs)
    assert calls == ["_sddmm", "_weighted"]
    calls.clear()
    assert not tiled.tiledEdgeScores(g.adj, A, B, heads=H).requires_grad
    calls.clear()
    L = gs.clone().requires_grad_(True)
    tiled.tiledEdgeSoftmax(g.adj, L).backward(gs)
    assert calls == ["_edge_softmax_grad"]
    calls.clear()
    assert not tiled.tiledEdgeSoftmax(g.adj, gs).requires_grad
    # the weighted sum: X's gradient alone is one sum on the other view, the weights' alone one per-edge dot
    tiled.tiledAggregate(g.adj, A.clone().requires_grad_(True), edge_weight=gs).sum().backward()
    assert calls == ["_weighted", "_weighted"]
    calls.clear()
    tiled.tiledAggregate(g.adj, A, edge_weight=gs.clone().requires_grad_(True)).sum().backward()
    assert calls == ["_weighted", "_sddmm"]
    calls.clear()
    # the attention with V alone: forward three launches, backward the sum on the other view only
    V = A.clone().requires_grad_(True)
    tiled.tiledEdgeAttention(g.adj, A, B, V, heads=H).sum().backward()
    assert calls == ["_sddmm", "_weighted", "_weighted"]
    # and there is no second derivative
    import torch

    X = A.clone().requires_grad_(True)
    gx, = torch.autograd.grad(tiled.tiledAggregate(g.adj, X, edge_weight=gs), X, A, create_graph=True)
    with pytest.raises(RuntimeError):
        gx.sum().backward()


@pytest.mark.parametrize("transposed", VIEWS)
def test_one_head_through_a_heads_entry_is_the_single_head_entry(transposed):
    """Every `*_heads*` entry of the C-ABI with heads = 1 against its single-head twin, bit for bit, on raw device pointers: the Python
    route sends one head through the heads entries, whose heads = 1 branch launches the single-head kernels."""
    torch = _torch()
    from qgtc_ppopp22_amd import cabi, tiled

    lib = cabi.load()
    g = graph(129)
    n, nnz = g.n, g.nnz
    head, idx = tiled._view_ptrs(view(g, transposed))
    rng = _rng(129, 8)

    def pair(*shape):   # two outputs that differ wherever an entry writes nothing
        return torch.zeros(shape, dtype=torch.float32, device="cuda"), torch.ones(shape, dtype=torch.float32, device="cuda")

    def ok(rc):
        assert rc == 0, lib.qgtc_strerror(rc).decode()

    for N in (5, 70):
        A, B = _dev(rng.normal(size=(n, N)).astype(np.float32)), _dev(rng.normal(size=(n, N)).astype(np.float32))
        v, r = _dev(rng.normal(size=nnz).astype(np.float32)), _dev(rng.uniform(0.5, 2.0, size=n).astype(np.float32))
        if not transposed:   # the per-edge dot has the row view only
            one, many = pair(nnz)
            ok(lib.qgtc_tiled_sddmm_f32(*head, A.data_ptr(), B.data_ptr(), A.numel(), N, *idx, one.data_ptr(), nnz, None))
            ok(lib.qgtc_tiled_sddmm_heads_f32(*head, A.data_ptr(), B.data_ptr(), A.numel(), N, *idx, many.data_ptr(), nnz, 1, None))
            assert same_bits(one, many), f"the per-edge dot, N={N}"
        mm, mm_heads = ((lib.qgtc_tiledmm_f32_t_edge, lib.qgtc_tiledmm_f32_t_edge_heads) if transposed else
                        (lib.qgtc_tiledmm_f32_edge, lib.qgtc_tiledmm_f32_edge_heads))
        for scale in (None, r.data_ptr()):
            one, many = pair(n, N)
            ok(mm(*head, A.data_ptr(), A.numel(), N, scale, one.data_ptr(), one.numel(), *idx, v.data_ptr(), nnz, None))
            ok(mm_heads(*head, A.data_ptr(), A.numel(), N, scale, many.data_ptr(), many.numel(), *idx, v.data_ptr(), nnz, 1, None))
            assert same_bits(one, many), f"the weighted sum, N={N}, row_scale {scale is not None}"
    ln = (3 * rng.normal(size=nnz)).astype(np.float32)
    ln[nnz // 2] = -np.inf
    L, G = _dev(ln), _dev(rng.normal(size=nnz).astype(np.float32))
    sm1, sm_heads, gr, gr_heads = ((lib.qgtc_tiled_edge_softmax_f32_t, lib.qgtc_tiled_edge_softmax_heads_f32_t,
                                    lib.qgtc_tiled_edge_softmax_grad_f32_t, lib.qgtc_tiled_edge_softmax_grad_heads_f32_t) if transposed else
                                   (lib.qgtc_tiled_edge_softmax_f32, lib.qgtc_tiled_edge_softmax_heads_f32,
                                    lib.qgtc_tiled_edge_softmax_grad_f32, lib.qgtc_tiled_edge_softmax_grad_heads_f32))
    (a1, ah), (m1, mh), (i1, ih), (d1, dh) = pair(nnz), pair(n), pair(n), pair(nnz)
    ok(sm1(*head, *idx, L.data_ptr(), a1.data_ptr(), nnz, m1.data_ptr(), i1.data_ptr(), None))
    ok(sm_heads(*head, *idx, L.data_ptr(), ah.data_ptr(), nnz, mh.data_ptr(), ih.data_ptr(), 1, None))
    assert same_bits(a1, ah) and same_bits(m1, mh) and same_bits(i1, ih), "the softmax and its statistics"
    ok(gr(*head, *idx, a1.data_ptr(), G.data_ptr(), d1.data_ptr(), nnz, None))
    ok(gr_heads(*head, *idx, a1.data_ptr(), G.data_ptr(), dh.data_ptr(), nnz, 1, None))
    assert same_bits(d1, dh), "the softmax gradient"


def _per_head_layer(layer, A, X):
    """conv.TransformerConv.forward as it was before the heads shared a call: a loop over the heads, from public single-head calls"""
    import torch
    from qgtc_ppopp22_amd import tiled

    Xn = A.to_new(X)
    q, k, v = torch.mm(Xn, layer.W_q), torch.mm(Xn, layer.W_k), torch.mm(Xn, layer.W_v)
    outs = []
    for i in range(layer.heads):
        cols = slice(i * layer.output_dim, (i + 1) * layer.output_dim)
        outs.append(tiled.tiledEdgeAttention(A, q[:, cols].contiguous(), k[:, cols].contiguous(), v[:, cols].contiguous()))
    out = torch.cat(outs, dim=1) if layer.concat else torch.stack(outs).mean(dim=0)
    return A.to_old(out)


@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("transposed", VIEWS)
@pytest.mark.parametrize("n,reorder", [(129, False), (300, True)])
def test_transformer_conv_equals_its_per_head_loop(n, reorder, transposed, concat):
    torch = _torch()
    from qgtc_ppopp22_amd.conv import TransformerConv

    g = graph(n, reorder)
    a = view(g, transposed)
    torch.manual_seed(n + concat)
    layer = TransformerConv(12, 7, heads=3, concat=concat).cuda()
    rng = _rng(n, 6)
    Xn = rng.normal(size=(n, 12)).astype(np.float32)
    dY = _dev(rng.normal(size=(n, 21 if concat else 7)).astype(np.float32))
    params = (layer.W_q, layer.W_k, layer.W_v)
    X = _dev(Xn).requires_grad_(True)
    Y = layer(a, X)
    got = torch.autograd.grad(Y, (X,) + params, dY)
    X2 = _dev(Xn).requires_grad_(True)
    Y2 = _per_head_layer(layer, a, X2)
    want = torch.autograd.grad(Y2, (X2,) + params, dY)
    assert Y.shape == (n, 21 if concat else 7) and same_bits(Y, Y2), "the output"
    for t, w, what in zip(got, want, ("dX", "dW_q", "dW_k", "dW_v")):
        assert same_bits(t, w), what


def test_refusals():
    torch = _torch()
    import QGTC
    from qgtc_ppopp22_amd import tiled

    g = graph(129)
    adj = g.adj
    rng = _rng(129, 7)
    X = _dev(rng.normal(size=(129, 12)).astype(np.float32))
    v = _dev(rng.normal(size=(g.nnz, 3)).astype(np.float32))
    bm = tiled.node_bitmap(torch.ones(g.n, dtype=torch.bool, device="cuda"), g.n)
    z = torch.zeros(g.n, device="cuda")
    for a in (adj, adj.T):
        # heads that do not divide the width, or are no positive int
        for bad in (5, 0, -1, 24):
            with pytest.raises(ValueError, match="heads"):
                tiled.tiledSDDMM(a, X, X, heads=bad)
            with pytest.raises(ValueError, match="heads"):
                tiled.tiledEdgeScores(a, X, X, heads=bad)
            with pytest.raises(ValueError, match="heads"):
                tiled.tiledEdgeAttention(a, X, X, X, heads=bad)
        with pytest.raises(TypeError):
            tiled.tiledSDDMM(a, X, X, heads=2.0)
        with pytest.raises(ValueError, match="heads"):
            tiled.tiledEdgeAttention(a, X, X, X[:, :10].contiguous(), heads=3)    # V's width
        for fn in (QGTC.tiledMMFloat, QGTC.tiledAggregate):
            with pytest.raises(ValueError, match="heads"):
                fn(a, X[:, :10].contiguous(), edge_weight=v)                      # 3 heads, 10 columns
            # whatever a 1-D edge_weight refuses, in the same words
            for kw in ({"src_scale": z}, {"edge_drop": (0.5, 1)}, {"row_mask": bm}, {"nbr_mask": bm}, {"reduce": "max"}, {"reduce": "min"},
                       {"attn": (z, z)}):
                with pytest.raises(ValueError) as two:
                    fn(a, X, edge_weight=v, **kw)
                with pytest.raises(ValueError) as one:
                    fn(a, X, edge_weight=v[:, 0].contiguous(), **kw)
                assert str(two.value) == str(one.value) and "not built" in str(two.value)
            with pytest.raises(ValueError):
                fn(a, X, edge_weight=v[:-1])                                      # a wrong length
            with pytest.raises(ValueError):
                fn(a, X, edge_weight=v[:, :, None])                               # a wrong shape
            with pytest.raises(TypeError):
                fn(a, X, edge_weight=v.double())                                  # a wrong dtype
            with pytest.raises(TypeError):
                fn(a, X, edge_weight=v.cpu().numpy())                             # not a tensor
            with pytest.raises(ValueError):
                fn(a, X, edge_weight=v.cpu())                                     # a wrong device
            with pytest.raises(ValueError):
                fn(a, X, edge_weight=torch.stack([v, v], 2)[:, :, 0])             # not contiguous
        with pytest.raises(ValueError):
            QGTC.tiledAggregate(a, X, row_scale=z.clone().requires_grad_(True), edge_weight=v)
        with pytest.raises(ValueError):
            tiled.tiledEdgeSoftmax(a, v[:-1])
        with pytest.raises(ValueError):
            tiled.tiledEdgeSoftmax(a, v[:, :, None])
        with pytest.raises(TypeError):
            tiled.tiledEdgeSoftmax(a, v.double())
        with pytest.raises(ValueError):
            tiled.tiledEdgeSoftmax(a, v.cpu())
        with pytest.raises(ValueError):
            tiled.tiledEdgeSoftmax(a, torch.stack([v, v], 2)[:, :, 0])
        with pytest.raises(ValueError):
            tiled.tiledSDDMM(a, X, X.t().contiguous().t(), heads=3)              # B's stride
        with pytest.raises(TypeError):
            tiled.tiledSDDMM(a, X, X.double(), heads=3)
        with pytest.raises(ValueError):
            tiled.tiledSDDMM(a, X, X.cpu(), heads=3)
