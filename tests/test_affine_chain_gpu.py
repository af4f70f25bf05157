"""The static affine chain on the GPU (``affine.linear`` / ``affine.aggregate`` with ``x_qparams=`` / ``t_qparams=``, uint8 operands and
``out=``; ``GCNConv_Affine.calibrate`` and ``forward(act_qparams=)`` over include/qgtc_chain.h) against tests/affine_model.py, bit for bit.
The reference multiplies codes in int64, dequantises with ``am.dequant``'s float steps and re-quantises with ``am.quantise``."""
import ctypes

import numpy as np
import pytest

import affine_model as am
import stream_cases as sc
from dirty_memory import same_as_model
from test_affine_dirty_gpu import _under_both_patterns
from test_affine_gpu import up, values
from test_affine_streams_gpu import RANGES, _content
from test_tiled_codes_gpu import LADDER, _hub_graph, _ladder_graph, _random_graph
from tiled_model import random_edges

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def env(qgtc, oracle):
    import torch
    from qgtc_ppopp22_amd import affine

    e = sc.env_of(qgtc, oracle, torch)
    e.af = affine
    return e


def row(scale, zp):
    """a caller's qparams row: (scale, zero point, 1 / scale, 0)"""
    return np.array([[scale, zp, F32(1) / F32(scale), 0]], F32)


def product(cx, qa, W, w, per_column=True, row_scale=None, bias=None, relu=False):
    """float32 [M, N]: the product of qgtc_linear.h on the codes cx of the left operand under the row qa (exact in int64 for any K)"""
    qb = am.qparams(W, w, per_column)
    cw = am.quantise(W, qb, w)
    t = cx.astype(np.int64) @ cw.astype(np.int64) + am.dequant_t(np.zeros((cx.shape[0], W.shape[1]), F32), cx.shape[1], qa, am.sums(cx, False),
                                                                  qb, am.sums(cw, True))
    s = (qa[0, 0] * np.broadcast_to(qb[:, 0], (W.shape[1],))).astype(F32)
    with np.errstate(over="ignore", invalid="ignore"):
        out = (t.astype(F32) * s[None, :]).astype(F32)
        if row_scale is not None:
            out = (out * row_scale[:, None]).astype(F32)
        if bias is not None:
            out = (out + bias[None, :]).astype(F32)
    return np.where(out > 0, out, F32(0)).astype(F32) if relu else out


def walk(A, cq, qt, row_scale=None, rm=None, nm=None):
    """float32 [n, N]: the fused walk of qgtc_codes.h on the codes cq under the row qt"""
    Am = am.masked_view(A, rm, nm)
    return am.dequant((Am @ cq.astype(np.int64)).astype(F32), A.shape[0], am.IDENTITY, Am.sum(axis=1), qt, None, row_scale)


def codes_on_device(env, c, ld=None, off=0, fill=0xFF):
    """the codes c [M, K] as a uint8 view with rows ld bytes apart, its base `off` bytes past a 256-byte boundary, every other byte `fill`"""
    M, K = c.shape
    ld = (K + 15) // 16 * 16 if ld is None else ld
    buf = env.torch.full((M * ld + 256,), fill, dtype=env.torch.uint8, device=env.dev)
    start = (-buf.data_ptr()) % 256 + off
    v = buf[start:start + M * ld].view(M, ld)[:, :K]
    v.copy_(up(env, c.astype(np.uint8)))
    return v


OUT8 = (8, row(0.37, 101.0))
SHAPES = ([(M, 65, 40) for M in (1, 15, 16, 17, 63, 64, 65, 130)] + [(17, 65, N) for N in (1, 15, 17, 64, 255, 257)] +
          [(17, K, 17) for K in (1, 3, 16, 63, 64, 130)] + [(17, 1100, 16), (17, 200, 256)])


@pytest.mark.parametrize("M,K,N", SHAPES, ids=str)
def test_the_three_products(env, M, K, N):
    """float -> codes, codes -> codes and codes -> float at every edge of the split; the code operand on the 16-byte path, on the dword
    path (ld = PAD4(K) + 4, base 4 bytes off) and with every pad byte 0xFF or 0: the result must not move"""
    rng = np.random.default_rng(M * 7919 + K * 31 + N)
    X, W = values(rng, M, K, 1), values(rng, K, N)
    qa = am.qparams(X, 8)
    cx = am.quantise(X, qa, 8)
    o = product(cx, qa, W, 4)
    qo = am.qparams(o * F32(0.5), 8)                                      # half of o's own range: both clamps are met
    want_q = am.quantise(o, qo, 8)
    dW, dqa, dout = up(env, W), up(env, qa), (8, up(env, qo))
    got = env.af.linear(up(env, X), dW, 8, 4, route="bytes", x_qparams=dqa, out=dout)
    assert got.dtype == env.torch.uint8 and (M == 1 or got.stride(0) % 16 == 0)
    same_as_model([got.cpu()], [want_q.astype(np.uint8)], f"float -> codes {M}x{K}x{N}")
    for how, kw in (("16-byte", {}), ("dword", {"ld": (K + 3) // 4 * 4 + 4, "off": 4}), ("zero pad", {"fill": 0})):
        dX = codes_on_device(env, cx, **kw)
        same_as_model([env.af.linear(dX, dW, 8, 4, route="bytes", x_qparams=dqa, out=dout).cpu()], [want_q.astype(np.uint8)],
                      f"codes -> codes {M}x{K}x{N} {how}")
        same_as_model([env.af.linear(dX, dW, 8, 4, route="bytes", x_qparams=dqa).cpu()], [o], f"codes -> float {M}x{K}x{N} {how}")


def _directed(rng, how):
    """(codes [M, K], qa, W, w_bits, keywords, out or None) of a case whose inputs are chosen; `check(o, q)` asserts the hit on the reference"""
    M, K, N = 33, 3, 21
    cx, qa, W, w, kw, out = rng.integers(0, 256, (M, K)), row(1.0, 0.0), rng.integers(0, 16, (K, N)).astype(F32), 4, {}, None
    W[0, 0], W[1, 0] = 0.0, 15.0                          # per tensor: scale 1, zero point 0, the codes are W itself
    check = lambda o, q: True                             # noqa: E731
    if how == "ties and clamps":                          # o = integers in -30 .. 105 under scale 2, zero point 3, 4 bits
        cx = rng.integers(0, 4, (M, K))
        kw, out = {"per_column": False, "bias": np.full(N, -30.0, F32)}, (4, row(2.0, 3.0))
        check = lambda o, q: (q == 0).any() and (q == 15).any() and ((np.abs(o * F32(0.5)) % 1 == 0.5) & (q > 0) & (q < 15)).any()   # noqa: E731
    elif how == "specials":
        rs = rng.normal(size=M).astype(F32)
        rs[:3] = np.nan, np.inf, -np.inf
        kw, out = {"row_scale": rs}, OUT8
        check = lambda o, q: np.isnan(o[0]).all() and (q[0] == 101).all() and set(q[1]) | set(q[2]) <= {0, 101, 255}   # noqa: E731
    elif how == "past 2^24":
        cx, W, w, K = np.full((M, 2048), 255), np.ones((2048, N), F32), 8, 2048
        W[0, :] = 0.0
        out = (8, row(2.0 ** 12, 7.0))
        check = lambda o, q: o.max() * 255 > 2 ** 24 and 0 < q.max() < 255   # noqa: E731
    elif how == "codes above a_bits":
        kw = {"a_bits": 3}
        check = lambda o, q: cx.max() > 7                 # noqa: E731
    elif how == "per tensor":
        kw = {"per_column": False}
    elif how == "bias and relu":
        kw = {"bias": rng.normal(size=N).astype(F32) * 100 - 500, "relu": True}
        check = lambda o, q: (o == 0).any() and (o > 0).any()   # noqa: E731
    return cx, qa, W, w, kw, out, check


@pytest.mark.parametrize("how", ["ties and clamps", "specials", "past 2^24", "codes above a_bits", "per tensor", "per column", "bias and relu"])
def test_directed_products(env, how):
    cx, qa, W, w, kw, out, check = _directed(np.random.default_rng(len(how)), how)
    a_bits = kw.pop("a_bits", 8)
    o = product(cx, qa, W, w, **kw)
    out = out or (8, am.qparams(o * F32(0.5), 8))         # half of o's own range unless the case fixes the row
    want = am.quantise(o, out[1], out[0])
    assert check(o, want) and len(np.unique(want)) > 1 or how == "past 2^24", how
    dkw = {k: up(env, v) if isinstance(v, np.ndarray) else v for k, v in kw.items()}
    for ld in (None, 4 * ((cx.shape[1] + 3) // 4) + 4):
        got = env.af.linear(codes_on_device(env, cx, ld), up(env, W), a_bits, w, route="bytes", x_qparams=up(env, qa), out=(out[0], up(env, out[1])),
                            **dkw)
        same_as_model([got.cpu()], [want.astype(np.uint8)], f"{how} ld={ld}")
    got = env.af.linear(codes_on_device(env, cx), up(env, W), a_bits, w, route="bytes", x_qparams=up(env, qa), **dkw)
    same_as_model([got.cpu()], [o], f"{how} as float")


@pytest.mark.parametrize("N", [5, 40])
def test_the_product_leaves_the_bytes_past_the_pad_alone(env, N):
    """qgtc_affine_linear_chain itself with ldo = PAD4(N) + 8 into canary bytes: codes, zeros up to PAD4(N), canaries beyond and around"""
    from qgtc_ppopp22_amd import cabi

    torch, M, K, ldo = env.torch, 70, 65, (N + 3) // 4 * 4 + 8
    X, W = (values(np.random.default_rng(N), *shape, 1) for shape in ((M, K), (K, N)))
    qa = am.qparams(X, 8)
    want = np.full((M + 2, ldo), 0xA5, np.uint8)
    want[1:M + 1, :(N + 3) // 4 * 4] = 0
    want[1:M + 1, :N] = am.quantise(product(am.quantise(X, qa, 8), qa, W, 4), OUT8[1], 8)
    buf = torch.full((M + 2, ldo), 0xA5, dtype=torch.uint8, device=env.dev)
    dX, dqa, dqo = up(env, X), up(env, qa), up(env, OUT8[1])
    wt, qb, cs = env.af.pack_weight(up(env, W), 4)
    rc = cabi.load().qgtc_affine_linear_chain(dX.data_ptr(), None, 0, 0, M, K, dqa.data_ptr(), 8, wt.data_ptr(), wt.size(1), wt.numel(), N,
                                              qb.data_ptr(), N, cs.data_ptr(), None, None, 0, None, 0, buf[1].data_ptr(), ldo,
                                              (M - 1) * ldo + (N + 3) // 4 * 4, dqo.data_ptr(), 8,
                                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    same_as_model([buf.cpu()], [want], f"canaries N={N} rc={rc}")


def test_the_static_calls_equal_the_composed_route(env):
    rng, n, K, N = np.random.default_rng(3), 200, 33, 24
    src, dst = (up(env, np.asarray(e, dtype=np.int64)) for e in random_edges(rng, n, 4 * n))
    adj = env.Q.pack_edges_tiled(src, dst, n)
    X, W, qo = up(env, values(rng, n, K, 1)), up(env, values(rng, K, N)), up(env, row(0.5, 60.0))
    af, qx = env.af, env.af.qparams(up(env, values(rng, n, K, 1)), 8)       # the row of another tensor: X clamps under it
    lin = af.linear(X, W, 8, 4, route="bytes", x_qparams=qx)
    same = lambda got, want, what: same_as_model([got.cpu()], [want.cpu().numpy()], what)   # noqa: E731
    same(af.linear(X, W, 8, 4, route="bytes", x_qparams=qx, out=(6, qo)), af.codes(lin, 6, qo), "linear(out=) against codes(linear())")
    same(af.linear(af.codes(X, 8, qx), W, 8, 4, route="bytes", x_qparams=qx), lin, "linear(uint8 X) against linear(float X)")
    for a in (adj, adj.T):
        agg = af.aggregate(a, lin, 8, a.mean_scale(), route="bytes", t_qparams=qx)
        same(af.aggregate(a, lin, 8, a.mean_scale(), route="bytes", t_qparams=qx, out=(6, qo)), af.codes(agg, 6, qo), "aggregate(out=)")
        same(af.aggregate(a, af.codes(lin, 8, qx), 8, a.mean_scale(), route="bytes", t_qparams=qx), agg, "aggregate(uint8 T)")


GRAPHS = {"random": lambda n, t: _random_graph(n, 5), "ladder": lambda n, t: _ladder_graph(n, t), "hub": lambda n, t: _hub_graph(n),
          "no edges": lambda n, t: (np.zeros(0, np.int64),) * 2}


@pytest.mark.parametrize("N", [3, 64, 100, 200])
@pytest.mark.parametrize("graph", GRAPHS)
def test_the_requantising_walks(env, graph, N):
    """codes -> codes on both views against the dense reference: unmasked, and under a row and a neighbour mask that leave whole blocks
    dead, on poisoned output; a row outside the mask or without neighbours is the zero point of the output row"""
    from qgtc_ppopp22_amd.tiled import node_bitmap

    n, rng = 700 if graph == "hub" else 300, np.random.default_rng(N)
    cq = np.full((n, N), 255) if graph == "hub" else rng.integers(0, 256, (n, N))
    qt, out = row(0.25, 37.0), (8, row(40.0 if graph == "hub" else 3.0, 11.0))
    rs = rng.random(n).astype(F32) + F32(0.5)
    rm, nm = rng.random(n) < 0.5, rng.random(n) < 0.5
    rm[:8], rm[128:256], nm[32:64] = True, False, False   # the ladder's rows stay; a k-quad of rows and a block of neighbours go
    dq, dqt, dout, drs = codes_on_device(env, cq, fill=0xEE), up(env, qt), (8, up(env, out[1])), up(env, rs)
    for transposed in (False, True):
        src, dst = GRAPHS[graph](n, transposed)
        A = am.dense_view(src, dst, n, transposed)
        if graph == "ladder":
            assert A.sum(axis=1)[:len(LADDER)].tolist() == list(LADDER)
        adj = env.Q.pack_edges_tiled(up(env, src), up(env, dst), n)
        a = adj.T if transposed else adj
        for masks, dm in ((None, {}), ((rm, nm), {"row_mask": node_bitmap(up(env, rm), n), "nbr_mask": node_bitmap(up(env, nm), n)})):
            want = am.quantise(walk(A, cq, qt, rs, *(masks or ())), out[1], 8)
            dead = am.masked_view(A, *(masks or ())).sum(axis=1) == 0
            assert (want[dead] == 11).all() and (dead.any() or not masks) and (graph == "no edges" or (want != 11).any())
            run = lambda: [env.af.aggregate(a, dq, 8, drs, route="bytes", t_qparams=dqt, out=dout, **dm)]   # noqa: E731,B023
            _under_both_patterns(env, f"walk {graph} N={N} T={transposed} masks={bool(masks)}", [dq], run, [want.astype(np.uint8)])


def test_the_products_on_poisoned_memory(env):
    rng = np.random.default_rng(1)
    X, W = values(rng, 70, 65, 1), values(rng, 65, 40)
    qa = am.qparams(X, 8)
    cx, o = am.quantise(X, qa, 8), product(am.quantise(X, qa, 8), qa, W, 4, relu=True)
    dX, dQ, dW, dqa, dqo = up(env, X), codes_on_device(env, cx), up(env, W), up(env, qa), up(env, OUT8[1])
    kw = {"route": "bytes", "relu": True, "x_qparams": dqa}
    run = lambda: [env.af.linear(dX, dW, 8, 4, out=(8, dqo), **kw), env.af.linear(dQ, dW, 8, 4, out=(8, dqo), **kw), env.af.linear(dQ, dW, 8, 4, **kw)]   # noqa: E731
    want_q = am.quantise(o, OUT8[1], 8).astype(np.uint8)
    _under_both_patterns(env, "the chain products", [dX, dQ, dW, dqa, dqo], run, [want_q, want_q, o])


def _layer(env, norm, seed=9, n=200):
    from qgtc_ppopp22_amd import conv

    rng = np.random.default_rng(seed)
    src, dst = random_edges(rng, n, 4 * n)
    adj = env.Q.pack_edges_tiled(up(env, np.asarray(src, np.int64)), up(env, np.asarray(dst, np.int64)), n)
    layer = env.af.GCNConv_Affine.from_float(conv.GCNConv(24, 16, 7, norm=norm).to(env.dev), 4, 8, route="bytes", linear_route="bytes")
    return rng, adj, am.dense_view(src, dst, n), layer


def chain_model(A, X, W_in, W_out, rows, norm, nodes=None):
    """the static layer in NumPy under the rows [4, 4]; X in the adjacency's numbering"""
    r, s = am.norm_scales(A, norm, nodes)
    q = [rows[i:i + 1] for i in range(4)]
    c = am.quantise(X, q[0], 8)
    c = am.quantise(product(c, q[0], W_in, 4, row_scale=s), q[1], 8)
    c = am.quantise(walk(A, c, q[1], r, nodes, nodes), q[2], 8)
    c = am.quantise(product(c, q[2], W_out, 4, row_scale=s), q[3], 8)
    return walk(A, c, q[3], r, nodes, nodes), c


@pytest.mark.parametrize("norm", [None, "mean", "sym"])
def test_the_static_layer(env, norm):
    rng, adj, A, layer = _layer(env, norm)
    n = A.shape[0]
    X, nodes = rng.normal(size=(n, 24)).astype(F32), rng.random(n) < 0.6
    for kw in ({}, {"nodes": up(env, nodes)}):
        rows = layer.calibrate(adj, up(env, X), **kw)
        assert tuple(rows.shape) == (4, 4) and not hasattr(layer, "act_qparams")
        same_as_model([layer(adj, up(env, X), act_qparams=rows, **kw).cpu()], [layer(adj, up(env, X), **kw).cpu().numpy()], f"static = dynamic {norm} {list(kw)}")
    # a second input three times as wide, under the rows of the first: against the NumPy chain, with clamping visible
    perm = adj.to_new(env.torch.arange(n, device=env.dev).view(n, 1).float()).cpu().numpy()[:, 0].astype(np.int64)   # new row i holds old row perm[i]
    rows, X2 = layer.calibrate(adj, up(env, X)), (X * 3).astype(F32)
    want, last = chain_model(A[np.ix_(perm, perm)], X2[perm], layer.W_in.detach().cpu().numpy(), layer.W_out.detach().cpu().numpy(), rows.cpu().numpy(), norm)
    assert ((last == 0) | (last == 255)).any() and (am.quantise(X2, rows.cpu().numpy()[:1], 8) == 255).any()
    same_as_model([layer(adj, up(env, X2), act_qparams=rows).cpu()], [want[np.argsort(perm)]], f"the clamping chain {norm}")


def test_refusals(env):
    _, adj, _, layer = _layer(env, None)
    t, af = env.torch, env.af
    X, W, qp = t.zeros((200, 24), device=env.dev), t.zeros((24, 8), device=env.dev), up(env, row(1.0, 0.0))
    layer.linear_route = "planes"
    bad = [(lambda kw=kw: af.linear(X, W, 8, 4, route="planes", **kw), "bytes") for kw in ({"x_qparams": qp}, {"out": (8, qp)})]
    bad += [(lambda kw=kw: af.aggregate(adj, X, 8, route="planes", **kw), "bytes") for kw in ({"t_qparams": qp}, {"out": (8, qp)})]
    bad += [(lambda: af.linear(X.to(t.uint8), W, 8, 4, route="bytes"), "x_qparams"), (lambda: layer.calibrate(adj, X), "bytes"),
            (lambda: af.linear(X.to(t.uint8), W, 9, 4, route="bytes", x_qparams=qp), "a_bits"),
            (lambda: layer(adj, X, act_qparams=t.zeros((4, 4), device=env.dev)), "bytes")]
    for call, match in bad:
        with pytest.raises(ValueError, match=match):
            call()


def test_the_static_layer_under_capture(env):
    """the rows are calibrated on the widest content, so every replay clamps differently and must follow its input"""
    rng, adj, A, layer = _layer(env, "mean", seed=4)
    n, torch = A.shape[0], env.torch
    contents, X = [[_content(rng, (n, 24), k)] for k in range(len(RANGES))], sc.empty(env, (n, 24), env.torch.float32)
    rows = layer.calibrate(adj, up(env, contents[1][0]))
    want = [[layer(adj, up(env, c[0]), act_qparams=rows).cpu().numpy()] for c in contents]
    assert not np.array_equal(want[0][0], want[3][0])
    live = sc.Live(torch, [X], contents, want, run=lambda: [layer(adj, X, act_qparams=rows)], keep=(adj, rows))
    sc.capture_and_replay(torch, env.Q, live, "GCNConv_Affine(act_qparams=)")
