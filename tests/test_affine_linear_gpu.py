"""The byte-code linear route on the GPU (``affine.pack_weight``, ``affine.linear(route="bytes")``, ``GCNConv_Affine(linear_route=)`` over
include/qgtc_linear.h) against tests/affine_model.py, bit for bit. The reference multiplies the model's codes in int64, so it is exact
past the 2^24 of the planes route; ``am.dequant`` takes its accumulator as float32, so beyond 2^24 its float steps are applied to the
int64 t here, and below 2^24 ``am.linear`` itself must agree. The shapes cross every edge of the kernel: the 16-row wave, the 64-row
workgroup, the 64-k step, the 16-column sub-tile, every sub-tile count compiled (1, 2, 4, 8, 16), a second LDS chunk at each (K > 1024,
704, 320, 128), a second column block (N > 256), and the scalar read (K % 4 != 0, or a base off 16 bytes)."""
import numpy as np
import pytest

import affine_model as am
import stream_cases as sc
from dirty_memory import same_as_model
from test_affine_dirty_gpu import _under_both_patterns
from test_affine_gpu import up, up_off4, values
from test_affine_streams_gpu import RANGES, _content
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


def model(X, W, a, w, per_column=True, row_scale=None, bias=None, relu=False):
    qa, qb = am.qparams(X, a), am.qparams(W, w, per_column)
    cx, cw = am.quantise(X, qa, a), am.quantise(W, qb, w)
    acc = cx.astype(np.int64) @ cw.astype(np.int64)
    t = acc + am.dequant_t(np.zeros(acc.shape, F32), X.shape[1], qa, am.sums(cx, False), qb, am.sums(cw, True))   # linear in acc: exact
    s = (qa[0, 0] * np.broadcast_to(qb[:, 0], (W.shape[1],))).astype(F32)
    out = (t.astype(F32) * s[None, :]).astype(F32)                                     # int64 -> float32 rounds to nearest even
    if row_scale is not None:
        out = (out * row_scale[:, None]).astype(F32)
    if bias is not None:
        out = (out + bias[None, :]).astype(F32)
    out = np.where(out > 0, out, F32(0)).astype(F32) if relu else out
    if acc.max(initial=0) < 2 ** 24:
        same_as_model([out], [am.linear(X, W, a, w, per_column, row_scale, bias, relu)], "the int64 reference against am.linear")
    return out


@pytest.mark.parametrize("K", [1, 15, 16, 17, 65])
@pytest.mark.parametrize("N", [1, 17])
def test_pack_weight(env, K, N):
    W = values(np.random.default_rng(K * 100 + N), K, N)
    W[K // 2, N // 2], W[0, 0], W[K - 1, N - 1] = np.nan, np.inf, -np.inf
    if N > 1:
        W[:, 3] = 0.0
    for bits in (1, 4, 8):
        for per_column in (True, False):
            qp = am.qparams(W, bits, per_column)
            q = am.quantise(W, qp, bits)
            want_t = np.zeros((N, (K + 15) // 16 * 16), np.uint8)
            want_t[:, :K] = q.T
            got = env.af.pack_weight(up(env, W), bits, per_column)
            same_as_model([g.cpu() for g in got], [want_t, qp, am.sums(q, True)], f"pack_weight {K}x{N} {bits} bits per_column={per_column}")
            same_as_model([got[1].cpu()], [env.af.qparams(up(env, W), bits, per_column).cpu().numpy()], "pack_weight's rows against affine.qparams")


PAIRS = [(1, 1), (8, 4), (4, 8), (8, 7), (8, 8)]
CASES = [(1, 1, 1, 1, 1, {}), (15, 3, 15, 8, 4, {}), (16, 63, 16, 4, 8, {}), (17, 64, 17, 8, 7, {}), (33, 65, 40, 8, 8, {}), (70, 130, 65, 8, 4, {}),
         *[(17, 65, 17, a, w, {}) for a, w in PAIRS],
         (16, 130, 130, 8, 4, {}), (17, 330, 65, 8, 8, {}), (1, 708, 40, 8, 4, {}), (16, 64, 260, 4, 8, {}),      # second chunk / column block
         *[(33, 65, 40, 8, 4, {k: True}) for k in ("row_scale", "bias", "relu", "per_tensor", "specials")],
         (33, 64, 40, 8, 4, {"off16": True}), (17, 300, 17, 8, 8, {"saturated": True}), (17, 2048, 17, 8, 8, {"qmax": True})]
PLANES_TOO = [(15, 3, 15), (17, 64, 17), (70, 130, 65)]


@pytest.mark.parametrize("M,K,N,a,w,how", CASES, ids=lambda v: ("-".join(v) or "plain") if isinstance(v, dict) else str(v))
def test_linear_bytes(env, M, K, N, a, w, how):
    rng = np.random.default_rng(M * 7919 + K * 31 + N + a)
    X, W = values(rng, M, K, 1), values(rng, K, N)
    if how.get("saturated"):                 # nine codes in ten are 0 or qmax (the ends of the range), the rest anything between
        X, W = (np.choose(rng.integers(0, 20, t.shape) // 9, [-50.0, 50.0, rng.uniform(-50, 50, t.shape)]).astype(F32) for t in (X, W))
    if how.get("qmax"):                      # every code 255: the sum is 2048 * 255^2
        X, W = np.ones((M, K), F32), np.ones((K, N), F32)
    if how.get("specials"):
        X[0, 0], X[M - 1, K - 1], X[M // 2, 1] = np.nan, np.inf, -np.inf
    kw = {"per_column": not how.get("per_tensor"), "relu": bool(how.get("relu")),
          "row_scale": rng.normal(size=M).astype(F32) if how.get("row_scale") else None, "bias": rng.normal(size=N).astype(F32) if how.get("bias") else None}
    dkw = {k: up(env, v) if isinstance(v, np.ndarray) else v for k, v in kw.items()}
    dX, dW = (up_off4 if how.get("off16") else up)(env, X), up(env, W)
    got = env.af.linear(dX, dW, a, w, route="bytes", **dkw)
    same_as_model([got.cpu()], [model(X, W, a, w, **kw)], f"linear bytes {M}x{K}x{N} ({a}, {w}) {how}")
    if (M, K, N) in PLANES_TOO and not how:
        same_as_model([got.cpu()], [env.af.linear(dX, dW, a, w, route="planes", **dkw).cpu().numpy()], "bytes against planes")


@pytest.mark.parametrize("norm", [None, "mean", "sym"])
def test_the_layer_with_both_linear_routes(env, norm):
    from qgtc_ppopp22_amd import conv

    torch, n = env.torch, 200
    rng = np.random.default_rng(9)
    src, dst = (up(env, np.asarray(e, dtype=np.int64)) for e in random_edges(rng, n, 4 * n))
    adj = env.Q.pack_edges_tiled(src, dst, n)
    layer = conv.GCNConv(24, 16, 7, norm=norm).to(env.dev)
    X, nodes = up(env, rng.normal(size=(n, 24)).astype(F32)), up(env, rng.random(n) < 0.6)
    by, pl = (env.af.GCNConv_Affine.from_float(layer, 4, 8, route="bytes", linear_route=r) for r in ("bytes", "planes"))
    for kw in ({}, {"nodes": nodes}):
        same_as_model([by(adj, X, **kw).cpu()], [pl(adj, X, **kw).cpu().numpy()], f"layer norm={norm} {list(kw)}")


def test_refusals(env):
    X, W = env.torch.zeros((1, 131072), device=env.dev), env.torch.zeros((131072, 1), device=env.dev)
    with pytest.raises(ValueError, match="131071"):
        env.af.linear(X, W, 8, 8, route="bytes")
    with pytest.raises(ValueError, match="route"):
        env.af.linear(X[:, :8].contiguous(), W[:8], 8, 8, route="bits")
    with pytest.raises(ValueError, match="linear_route"):
        env.af.GCNConv_Affine(4, 4, 4, linear_route="bits")


@pytest.fixture(scope="module")
def live(env):
    """X [70, 65] and W [65, 40] in four ranges (a replay must follow scale and zero point), and the model's result on each"""
    torch, rng = env.torch, np.random.default_rng(11)
    contents = [[_content(rng, (70, 65), k), _content(rng, (65, 40), (k + 1) % 4)] for k in range(len(RANGES))]
    X, W = sc.empty(env, (70, 65), torch.float32), sc.empty(env, (65, 40), torch.float32)
    return sc.Live(torch, [X, W], contents, [[model(x, w, 8, 4, relu=True)] for x, w in contents],
                   run=lambda: [env.af.linear(X, W, 8, 4, route="bytes", relu=True)])


def test_linear_bytes_under_capture(env, live):
    sc.capture_and_replay(env.torch, env.Q, live, "linear(route='bytes')")


def test_linear_bytes_on_dirty_memory(env, live):
    live.load(1)
    env.torch.cuda.synchronize(env.dev)
    _under_both_patterns(env, "linear(route='bytes')", live.bufs, live.run, live.expected[1])
