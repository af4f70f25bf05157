"""The fused middle of the static affine chain on the GPU (``affine.aggregate_linear``, ``GCNConv_Affine.forward(fuse=True)`` over
include/qgtc_fused.h), bit for bit against tests/affine_model.py composed in NumPy (int64 neighbour sums, dequant, quantise under h,
the int64 product, dequant, quantise under out) and against the composed device route ``linear(aggregate(..., out=h), ...)``."""
import ctypes

import numpy as np
import pytest

import affine_model as am
import stream_cases as sc
from dirty_memory import same_as_model
from test_affine_chain_gpu import OUT8, _layer, codes_on_device, env, product, row, walk  # noqa: F401
from test_affine_dirty_gpu import _under_both_patterns
from test_affine_gpu import up, values
from test_affine_streams_gpu import RANGES, _content
from test_tiled_codes_gpu import _hub_graph, _ladder_graph, _random_graph

pytestmark = pytest.mark.gpu
F32 = np.float32
H8 = (8, row(0.75, 9.0))


def both_routes(env, adj, A, cq, qt, h, W, out, ars=None, lrs=None, masks=None, **kw):
    """([fused], [the NumPy chain], [the composed device route]) of one case; kw: per_column, bias, relu"""
    rm, nm = masks or (None, None)
    o = product(am.quantise(walk(A, cq, qt, ars, rm, nm), h[1], h[0]), h[1], W, 4, row_scale=lrs, **kw)
    want = o if out is None else am.quantise(o, out[1], out[0]).astype(np.uint8)
    d = lambda v: up(env, v) if isinstance(v, np.ndarray) else v   # noqa: E731
    dkw, dm = {k: d(v) for k, v in kw.items()}, {}
    if masks:
        from qgtc_ppopp22_amd.tiled import node_bitmap
        dm = {"row_mask": node_bitmap(up(env, rm), len(rm)), "nbr_mask": node_bitmap(up(env, nm), len(nm))}
    dq, dqt, dh, dW = codes_on_device(env, cq, fill=0xFF), up(env, qt), (h[0], up(env, h[1])), up(env, W)
    dout, dars, dlrs = out and (out[0], up(env, out[1])), d(ars), d(lrs)
    fused = lambda: [env.af.aggregate_linear(adj, dq, dqt, dh, dW, 4, agg_row_scale=dars, lin_row_scale=dlrs, out=dout, **dkw, **dm)]   # noqa: E731
    hq = env.af.aggregate(adj, dq, 8, dars, route="bytes", t_qparams=dqt, out=dh, **dm)
    two = env.af.linear(hq, dW, h[0], 4, row_scale=dlrs, route="bytes", x_qparams=dh[1], out=dout, **dkw)
    return fused, want, two.cpu().numpy()


SHAPES = [("random", 70, 3, 40), ("random", 70, 64, 1), ("random", 70, 65, 16), ("random", 70, 100, 17), ("random", 70, 200, 100),
          ("random", 70, 256, 256), ("random", 70, 128, 256), ("random", 33, 64, 40), ("ladder", 300, 100, 40), ("hub", 700, 64, 17)]


@pytest.mark.parametrize("graph,n,K,N2", SHAPES, ids=str)
def test_the_fused_launch(env, graph, n, K, N2):
    rng = np.random.default_rng(n * 7919 + K * 31 + N2)
    src, dst = {"random": lambda: _random_graph(n, 5), "ladder": lambda: _ladder_graph(n, False), "hub": lambda: _hub_graph(n)}[graph]()
    A, adj = am.dense_view(src, dst, n), env.Q.pack_edges_tiled(up(env, src), up(env, dst), n)
    cq = np.full((n, K), 255) if graph == "hub" else rng.integers(0, 256, (n, K))
    qt, W, ars = row(0.25, 37.0), values(rng, K, N2), rng.random(n).astype(F32) + F32(0.5)
    h = (8, am.qparams(walk(A, cq, qt, ars) * F32(0.5), 8))           # half of the intermediate's own range: both clamps are met
    assert graph != "hub" or (A @ cq).max() > 2 ** 16
    for out in (None, OUT8):
        fused, want, two = both_routes(env, adj, A, cq, qt, h, W, out, ars)
        got = fused()[0]
        assert out is None or (got.dtype == env.torch.uint8 and got.stride(0) % 16 == 0)
        same_as_model([got.cpu()], [want], f"fused against the NumPy chain {graph} {n}x{K}x{N2} out={out is not None}")
        same_as_model([got.cpu()], [two], f"fused against the two launches {graph} {n}x{K}x{N2} out={out is not None}")


@pytest.mark.parametrize("how", ["no edges", "masks"])
@pytest.mark.parametrize("per_column", [False, True])
def test_directed_on_poisoned_memory(env, how, per_column):
    """rows that sum nothing still run the product: a graph without edges; a dead 32-row block and a masked row in a live block"""
    n, K, N2, rng = 100, 65, 21, np.random.default_rng(11)
    src, dst = (np.zeros(0, np.int64),) * 2 if how == "no edges" else _random_graph(n, 5)
    A, adj = am.dense_view(src, dst, n), env.Q.pack_edges_tiled(up(env, src), up(env, dst), n)
    rm, nm = np.ones(n, bool), rng.random(n) < 0.7
    rm[32:64], rm[70] = False, False
    ars, lrs = rng.random(n).astype(F32) + F32(0.5), rng.normal(size=n).astype(F32)
    ars[40], ars[70], ars[3] = np.nan, np.inf, np.inf                 # in the dead block, on the masked row, on a live row
    kw = {"per_column": per_column, "bias": rng.normal(size=N2).astype(F32) * 20, "relu": True}
    for out in (None, OUT8):
        fused, want, two = both_routes(env, adj, A, rng.integers(0, 256, (n, K)), row(0.25, 37.0), H8, values(rng, K, N2), out, ars, lrs,
                                       (rm, nm) if how == "masks" else None, **kw)
        same_as_model([want], [two], f"the model against the two launches ({how})")
        _under_both_patterns(env, f"fused {how} per_column={per_column} out={out is not None}", [], fused, [two])


@pytest.mark.parametrize("norm", [None, "mean", "sym"])
def test_the_fused_layer_is_the_static_layer(env, norm):
    rng, adj, A, layer = _layer(env, norm)
    X, nodes = up(env, rng.normal(size=(A.shape[0], 24)).astype(F32)), up(env, rng.random(A.shape[0]) < 0.6)
    for kw in ({}, {"nodes": nodes}):
        rows = layer.calibrate(adj, X, **kw)
        same_as_model([layer(adj, X * 3, act_qparams=rows, fuse=True, **kw).cpu()], [layer(adj, X * 3, act_qparams=rows, **kw).cpu().numpy()],
                      f"fuse=True against fuse=False {norm} {list(kw)}")


def test_the_fused_layer_under_capture(env):
    rng, adj, A, layer = _layer(env, "mean", seed=4)
    n, torch = A.shape[0], env.torch
    contents, X = [[_content(rng, (n, 24), k)] for k in range(len(RANGES))], sc.empty(env, (n, 24), env.torch.float32)
    rows = layer.calibrate(adj, up(env, contents[1][0]))
    want = [[layer(adj, up(env, c[0]), act_qparams=rows).cpu().numpy()] for c in contents]
    live = sc.Live(torch, [X], contents, want, run=lambda: [layer(adj, X, act_qparams=rows, fuse=True)], keep=(adj, rows))
    sc.capture_and_replay(torch, env.Q, live, "GCNConv_Affine(act_qparams=, fuse=True)")


@pytest.mark.parametrize("N2", [5, 40])
def test_the_entry_leaves_the_bytes_past_the_pad_alone(env, N2):
    """qgtc_tiledmm_u8_linear itself with ldo = PAD4(N2) + 8 into canary bytes: codes, zeros up to PAD4(N2), canaries beyond and around"""
    from qgtc_ppopp22_amd import cabi, tiled

    torch, n, K, ldo, rng = env.torch, 70, 65, (N2 + 3) // 4 * 4 + 8, np.random.default_rng(N2)
    src, dst = _random_graph(n, 5)
    adj, cq, W, qt = env.Q.pack_edges_tiled(up(env, src), up(env, dst), n), rng.integers(0, 256, (n, K)), values(rng, K, N2), row(0.25, 37.0)
    want = np.full((n + 2, ldo), 0xA5, np.uint8)
    want[1:n + 1, :(N2 + 3) // 4 * 4] = 0
    want[1:n + 1, :N2] = am.quantise(product(am.quantise(walk(am.dense_view(src, dst, n), cq, qt), H8[1], 8), H8[1], W, 4), OUT8[1], 8)
    buf = torch.full((n + 2, ldo), 0xA5, dtype=torch.uint8, device=env.dev)
    dq, dqt, dh, dqo = codes_on_device(env, cq), up(env, qt), up(env, H8[1]), up(env, OUT8[1])
    wt, qb, cs = env.af.pack_weight(up(env, W), 4)
    rc = cabi.load().qgtc_tiledmm_u8_linear(*tiled._view_args(adj), dq.data_ptr(), dq.stride(0), n * dq.stride(0), K, dqt.data_ptr(), None,
                                            dh.data_ptr(), 8, wt.data_ptr(), wt.size(1), wt.numel(), N2, qb.data_ptr(), N2, cs.data_ptr(), None,
                                            None, 0, None, 0, buf[1].data_ptr(), ldo, (n - 1) * ldo + (N2 + 3) // 4 * 4, dqo.data_ptr(), 8, None,
                                            None, 0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    same_as_model([buf.cpu()], [want], f"canaries N2={N2} rc={rc}")


def test_refusals(env):
    _, adj, _, layer = _layer(env, None)
    t, qp = env.torch, up(env, row(1.0, 0.0))
    T = lambda K: t.zeros((200, K), dtype=t.uint8, device=env.dev)    # noqa: E731
    W = lambda K, N: t.zeros((K, N), device=env.dev)                 # noqa: E731
    for call in (lambda: env.af.aggregate_linear(adj.T, T(24), qp, (8, qp), W(24, 8), 4), lambda: env.af.aggregate_linear(adj, T(257), qp, (8, qp), W(257, 8), 4),
                 lambda: env.af.aggregate_linear(adj, T(24), qp, (8, qp), W(24, 257), 4)):
        with pytest.raises(ValueError, match=r"aggregate\(.*linear\("):
            call()
    with pytest.raises(ValueError, match="act_qparams"):
        layer(adj, t.zeros((200, 24), device=env.dev), fuse=True)
