"""The edge-weighted sum on byte codes on the device (``affine.aggregate(route="bytes", edge_weight=)``, the two C entries of
include/qgtc_codes_edge.h, ``affine.TransformerConv_Affine`` and ``affine.GATv2Conv_Affine``) against inline NumPy float64 on the dense
masked view: ((A * Wd) @ (Q - z)) * scale * row_scale per head. The weights come from an edge list through ``tiled.edge_values``, so the
reference never touches slot order. Both views in every test."""
import ctypes
import math

import numpy as np
import pytest

import affine_model as am
from test_tiled_codes_gpu import _bm, _dev, _hub_graph, _ladder_graph, _random_graph, af  # noqa: F401

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
NO_EDGES = (np.zeros(0, np.int64), np.zeros(0, np.int64))
# (n, N, graph, heads): every width class and dwords that straddle N; block and k-quad edges; degrees across the queue; the head shapes
CASES = ([(300, N, "random", 1) for N in (1, 3, 4, 5, 64, 65, 256, 257, 300)] + [(n, N, "random", 1) for n in (1, 31, 32, 33, 127, 128, 129) for N in (5, 64)]
         + [(300, 64, g, 1) for g in ("ladder", "hub", "none")] + [(300, H * d, "random", H) for H, d in ((2, 4), (8, 8), (4, 16), (3, 12))]
         + [(300, 36, "ladder", 3), (300, 64, "hub", 8)])


def _setup(qgtc, n, graph, t, H, seed, draw):
    """(the view, its dense 0 / 1 matrix, its dense weights [H, n, n], edge_weight on the device) of a graph without repeated edges;
    ``draw(rng, key)`` gives one head's weights, ``key`` the view's row of every edge"""
    import torch
    from qgtc_ppopp22_amd import tiled

    src, dst = {"random": lambda: _random_graph(n, seed), "ladder": lambda: _ladder_graph(n, t), "hub": lambda: _hub_graph(n), "none": lambda: NO_EDGES}[graph]()
    cells = np.unique(src * n + dst)
    src, dst = cells // n, cells % n
    adj = qgtc.pack_edges_tiled(_dev(src), _dev(dst), n)
    rng = np.random.default_rng(seed + 1)
    w = [draw(rng, dst if t else src).astype(F32) for _ in range(H)]
    Wd = np.zeros((H, n, n), F64)
    for h in range(H):
        Wd[h, src, dst] = w[h]
    vals = [tiled.edge_values(adj, _dev(src), _dev(dst), _dev(x)) for x in w]
    ew = vals[0] if H == 1 else torch.stack(vals, 1).contiguous()
    return (adj.T if t else adj), am.dense_view(src, dst, n, t), (Wd.transpose(0, 2, 1) if t else Wd), ew


# one head's weights of the edges whose row of the view is ``key``: eighths in [-4, 4], signed normals, rows that sum to 1
EIGHTHS = lambda rng, key: rng.integers(-32, 33, key.size) / 8.0   # noqa: E731
NORMAL = lambda rng, key: rng.normal(size=key.size)   # noqa: E731
SOFTMAX = lambda rng, key: (lambda e: e / np.bincount(key, e)[key])(np.exp(rng.normal(size=key.size)))   # noqa: E731


def _ref(A, Wd, Q, qp, rs):
    """(float64 [n, N] of the definition, the bound's sum |w| per row and column) on the masked view A"""
    H, d = Wd.shape[0], Q.shape[1] // Wd.shape[0]
    x = Q.astype(F64) - F64(qp[0, 1])
    y = np.concatenate([(A * Wd[h]) @ x[:, h * d:(h + 1) * d] for h in range(H)], 1) * F64(qp[0, 0])
    absw = np.repeat(np.stack([(A * np.abs(Wd[h])).sum(1) for h in range(H)], 1), d, 1)
    return (y if rs is None else y * rs.astype(F64)[:, None]), absw


def _padded(Q):
    """Q on the device as a view of a buffer whose pad bytes hold 0xFF: a surplus byte that leaked would show"""
    buf = np.full((Q.shape[0], (Q.shape[1] + 3) // 4 * 4 + 4), 0xFF, np.uint8)
    buf[:, :Q.shape[1]] = Q
    return _dev(buf)[:, :Q.shape[1]]


@pytest.mark.parametrize("n,N,graph,H", CASES, ids=[f"n{n}-N{N}-{g}-H{H}" for n, N, g, H in CASES])
def test_exact_on_eighths(af, qgtc, n, N, graph, H):
    """weights in eighths in [-4, 4], (scale, z) = (0.5, integer), row scales powers of two: every partial sum is below 2^24 eighths at
    degree <= 300, so float32 is exact in any order, fused or not - equality with float64, and the code output bit for bit"""
    rng = np.random.default_rng(n * 1000 + N)
    Q = rng.integers(0, 256, (n, N)).astype(np.uint8)
    qp = np.array([[0.5, rng.integers(0, 256), 2.0, 0.0]], F32)
    rs = (2.0 ** rng.integers(-2, 3, n)).astype(F32)
    oqp = np.array([[3.0, 100.0, 1.0 / 3.0, 0.0]], F32)
    R, S = rng.random(n) < 0.5, rng.random(n) < 0.5           # a random half: slots must be counted on the raw words
    for t in (False, True):
        a, A, Wd, ew = _setup(qgtc, n, graph, t, H, 7 + n, EIGHTHS)
        for rm, sm in ((None, None), (R, S)):
            kw = dict(route="bytes", t_qparams=_dev(qp), edge_weight=ew, row_mask=_bm(rm, n), nbr_mask=_bm(sm, n))
            want, _ = _ref(am.masked_view(A, rm, sm), Wd, Q, qp, rs)
            y = af.aggregate(a, _padded(Q), 8, _dev(rs), **kw)
            assert (y.cpu().numpy().astype(F64) == want).all() and not np.signbit(y.cpu().numpy()[want == 0]).any(), f"transposed={t} masks={rm is not None}"
            q = af.aggregate(a, _padded(Q), 8, _dev(rs), out=(8, _dev(oqp)), **kw)
            assert q.data_ptr() % 16 == 0 and (q.cpu() == af.codes(y, 8, _dev(oqp)).cpu()).all(), "the code output"


def test_the_raw_entry_on_a_strided_destination(af, qgtc):
    """codes into rows PAD4(N) + 8 apart of a buffer of canaries: codes, zeros up to PAD4(N), canaries beyond"""
    import torch
    from qgtc_ppopp22_amd import cabi, tiled

    n, N, H, ldo = 130, 22, 1, 32
    Q = np.random.default_rng(3).integers(0, 256, (n, N)).astype(np.uint8)
    qp, oqp = _dev(np.array([[0.5, 9.0, 2.0, 0.0]], F32)), _dev(np.array([[2.0, 128.0, 0.5, 0.0]], F32))
    for t in (False, True):
        a, _, _, ew = _setup(qgtc, n, "random", t, H, 5, EIGHTHS)
        dQ, out = _padded(Q), torch.full((n, ldo), 0xA5, dtype=torch.uint8, device="cuda")
        val_ptr, val_row, nnz = tiled._value_index(a)
        rc = getattr(cabi.load(), "qgtc_tiledmm_u8" + ("_t" if t else "") + "_edge")(
            *tiled._view_args(a), dQ.data_ptr(), dQ.stride(0), (n - 1) * dQ.stride(0) + 24, N, qp.data_ptr(), None, val_ptr.data_ptr(),
            val_row.data_ptr(), ew.data_ptr(), nnz, H, None, 0, out.data_ptr(), ldo, (n - 1) * ldo + 24, oqp.data_ptr(), 8, None, None, 0,
            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
        whole = out.cpu().numpy()
        want = af.aggregate(a, dQ, 8, route="bytes", t_qparams=qp, edge_weight=ew, out=(8, oqp)).cpu().numpy()
        assert (whole[:, :N] == want).all() and (whole[:, N:24] == 0).all() and (whole[:, 24:] == 0xA5).all()


@pytest.mark.parametrize("draw", [SOFTMAX, NORMAL], ids=["softmax", "normal"])
@pytest.mark.parametrize("n,N,graph,H", [(300, 65, "random", 1), (300, 64, "hub", 8), (300, 36, "ladder", 3), (129, 257, "random", 1)], ids=str)
def test_within_the_derived_bound(af, qgtc, n, N, graph, H, draw):
    """random float weights and codes, arbitrary qparams (float T: the dynamic route): with T_o live terms
    |y - y64| <= (T_o + 4) 2^-23 scale |row_scale_o| (255 + z) sum_k |w| - at most two roundings a term on magnitudes <= 255 sum |w|, one
    a term on sum w, four in the epilogue"""
    import torch

    rng = np.random.default_rng(n + N)
    T = (rng.normal(size=(n, N)) * 3.0 - 1.0).astype(F32)
    rs = rng.normal(size=n).astype(F32)
    R, S = rng.random(n) < 0.6, rng.random(n) < 0.6
    for t in (False, True):
        a, A, Wd, ew = _setup(qgtc, n, graph, t, H, 11 + N, draw)
        qp = af.qparams(_dev(T), 8)
        Q = af.codes(_dev(T), 8, qp)
        for scale, (rm, sm) in ((None, (None, None)), (rs, (R, S))):
            Am = am.masked_view(A, rm, sm)
            want, absw = _ref(Am, Wd, Q.cpu().numpy(), qp.cpu().numpy(), scale)
            y = af.aggregate(a, _dev(T), 8, None if scale is None else _dev(scale), route="bytes", edge_weight=ew, row_mask=_bm(rm, n),
                             nbr_mask=_bm(sm, n))
            same = af.aggregate(a, Q, 8, None if scale is None else _dev(scale), route="bytes", t_qparams=qp, edge_weight=ew,
                                row_mask=_bm(rm, n), nbr_mask=_bm(sm, n))
            assert torch.equal(y, same), "float T is qparams + codes + the walk on them"
            s, z = (F64(v) for v in qp.cpu().numpy()[0, :2])
            bound = (Am.sum(1) + 4)[:, None] * 2.0 ** -23 * s * (1.0 if scale is None else np.abs(scale.astype(F64))[:, None]) * (255 + z) * absw
            err = np.abs(y.cpu().numpy().astype(F64) - want)
            print(f"{graph} t={t} masks={rm is not None}: max err / bound = {np.max(err / np.maximum(bound, 1e-300)):.3g}")
            assert (err <= bound).all()


def test_the_refusals(af, qgtc):
    import torch

    n, N = 40, 12
    a, _, _, ew = _setup(qgtc, n, "random", False, 1, 2, NORMAL)
    T = torch.ones((n, N), dtype=torch.float32, device="cuda")
    for kw, err in ((dict(route="planes"), ValueError), (dict(route="bytes", reduce="max"), ValueError), (dict(edge_weight=ew[:-1]), ValueError),
                    (dict(edge_weight=ew.double()), TypeError), (dict(edge_weight=ew.cpu()), ValueError),
                    (dict(edge_weight=torch.stack([ew] * 5, 1).contiguous()), ValueError)):
        with pytest.raises(err):
            af.aggregate(a, T, 8, **{"route": "bytes", "edge_weight": ew, **kw})
    with pytest.raises(ValueError, match="tiledAggregate"):     # 2 heads of 6 columns
        af.aggregate(a, T, 8, route="bytes", edge_weight=torch.stack([ew] * 2, 1).contiguous())


def _compose(af, layer, A, X, nodes):
    """the forward of either layer as the public calls it is specified to be"""
    from qgtc_ppopp22_amd import conv, tiled

    Xn = A.to_new(X).contiguous()
    lin = lambda W: af.linear(Xn, W.detach().contiguous(), layer.act_bit, layer.w_bit, route="bytes")   # noqa: E731
    if isinstance(layer, af.TransformerConv_Affine):
        V, logits = lin(layer.W_v), tiled.tiledEdgeScores(A, lin(layer.W_q), lin(layer.W_k), layer.heads) * (1.0 / math.sqrt(layer.output_dim))
    else:
        V = lin(layer.W_l)
        logits = tiled.tiledEdgeAdditiveScores(A, V if layer.share_weights else lin(layer.W_r), V, layer.att.detach(), layer.negative_slope, layer.heads)
    bm = None if nodes is None else conv._node_mask(A, nodes)
    out = af.aggregate(A, V, layer.act_bit, route="bytes", edge_weight=tiled.tiledEdgeSoftmax(A, logits), row_mask=bm, nbr_mask=bm)
    if layer.heads > 1 and not layer.concat:
        out = out.view(A.n, layer.heads, layer.output_dim).transpose(0, 1).contiguous().mean(dim=0)
    return A.to_old(out)


@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("heads", [1, 4])
@pytest.mark.parametrize("name", ["TransformerConv", "GATv2Conv", "GATv2Conv-shared"])
def test_the_layers_are_the_composition_of_the_public_calls(af, qgtc, name, heads, concat):
    import torch
    from qgtc_ppopp22_amd import conv

    n, f, d = 200, 10, 8
    src, dst = _random_graph(n, 31)
    adj = qgtc.pack_edges_tiled(_dev(src), _dev(dst), n, reorder=True)
    torch.manual_seed(heads)
    if name == "TransformerConv":
        fl, cls, names = conv.TransformerConv(f, d, heads, concat).cuda(), af.TransformerConv_Affine, ("W_q", "W_k", "W_v")
    else:
        fl = conv.GATv2Conv(f, d, heads, 0.3, concat, share_weights=name.endswith("shared")).cuda()
        cls, names = af.GATv2Conv_Affine, ("W_l", "att", "negative_slope", "share_weights") + (() if fl.share_weights else ("W_r",))
    layer = cls.from_float(fl, 4, 8)
    for k in names + ("heads", "concat", "input_dim", "output_dim"):
        x, y = getattr(fl, k), getattr(layer, k)
        assert (torch.equal(x, y) and x is not y) if isinstance(x, torch.Tensor) else x == y, k
    assert (layer.w_bit, layer.act_bit) == (4, 8)
    X, nodes = torch.randn(n, f, device="cuda"), torch.rand(n, device="cuda") < 0.6
    for A in (adj, adj.T):
        for nd in (None, nodes):
            y = layer(A, X, nodes=nd)
            assert tuple(y.shape) == (n, d * (heads if concat else 1)) and not y.requires_grad
            assert torch.equal(y, _compose(af, layer, A, X, nd)), f"transposed={A.transposed} nodes={nd is not None}"
            assert nd is None or not y[~nd].any()


def test_replays_of_a_captured_aggregate_follow_the_weights(af, qgtc):
    import torch

    n, N, H = 300, 64, 4
    Q = _dev(np.random.default_rng(1).integers(0, 256, (n, N)).astype(np.uint8))
    qp = _dev(np.array([[0.25, 17.0, 4.0, 0.0]], F32))
    a, _, _, ew = _setup(qgtc, n, "random", False, H, 41, NORMAL)
    views = (a, a.T)                                           # one adjacency, one weight array: slot order is the tiles'
    weights = [torch.randn_like(ew) for _ in range(3)]
    eager = [[af.aggregate(v, Q, 8, route="bytes", t_qparams=qp, edge_weight=w) for v in views] for w in weights]   # (also the warm-up)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ys = [af.aggregate(v, Q, 8, route="bytes", t_qparams=qp, edge_weight=ew) for v in views]
    for k in (1, 2, 0, 2):
        ew.copy_(weights[k])
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(y, e) for y, e in zip(ys, eager[k])), f"replay of weights {k}"
