"""The byte-code route on recycled, poisoned device memory (tests/dirty_memory.py; DESIGN.md, "Dirty memory"): the code buffer with its
pad bytes, the int sums, the fused aggregate's output and the padded copy of a misaligned code matrix all come from ``torch.empty``.
``codes``, ``tiledMMCodes``, ``aggregate(route="bytes")`` and the layer run under ``dirty`` once per pattern; every word must equal
tests/tiled_codes_model.py bit for bit, and the two patterns' results each other."""
import numpy as np
import pytest

import affine_model as am
import dirty_memory as dm
import stream_cases as sc
import tiled_codes_model as cm
import tiled_nodes_model as nm
from tiled_model import random_edges

pytestmark = pytest.mark.gpu
F32 = np.float32
MODULE = "tests/test_tiled_codes_dirty_gpu.py"


@pytest.fixture(scope="module")
def env(qgtc, oracle):
    import torch
    from qgtc_ppopp22_amd import affine

    e = sc.env_of(qgtc, oracle, torch)
    e.af = affine
    return e


def _under_both_patterns(env, what, inputs, run, want):
    torch, results = env.torch, []
    for pattern in dm.PATTERNS:
        with dm.dirty(torch, env.dev, pattern, inputs=inputs) as d:
            dm.announce(MODULE, d)
            got = [t.detach().cpu() for t in run()]
        dm.same_as_model(got, want, f"{what} on memory poisoned with {pattern:#010x}")
        results.append(got)
    dm.same_bits(results[0], results[1], f"{what}: {dm.PATTERNS[0]:#010x} against {dm.PATTERNS[1]:#010x}")


def _up(env, a):
    a = np.ascontiguousarray(a)
    return env.torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(env.dev)


def _x(shape, seed):
    rng = np.random.default_rng(seed)
    x = (rng.normal(size=shape) * 3.0 - 1.0).astype(F32)
    x[rng.integers(0, shape[0]), rng.integers(0, shape[1])] = np.nan
    return x


def _graph(n):
    return tuple(np.asarray(a, dtype=np.int64) for a in random_edges(np.random.default_rng(70 + n), n, 3 * n))


@pytest.mark.parametrize("shape", [(33, 130), (100, 7), (257, 64)], ids=str)
def test_codes_on_dirty_memory(env, shape):
    x = _x(shape, 1)
    dx = _up(env, x)
    H, W = shape
    for bits in (3, 8):
        want, d_qp = [], []
        for per_column in (False, True):
            qp = am.qparams(x, bits, per_column)
            want.append(cm.codes_buffer(x, qp, bits))            # the pad bytes up to PAD4(W) are written: zeros, not poison
            d_qp.append(_up(env, qp))

        def run():
            return [env.af.codes(dx, bits, qp).as_strided((H, cm.pad4(W)), (cm.pad4(W), 1)) for qp in d_qp]

        run()                                                    # outside the poisoned region: code objects are loaded
        _under_both_patterns(env, f"codes {shape} {bits} bits", [dx] + d_qp, run, want)


@pytest.mark.parametrize("transposed", [False, True], ids=["adj", "adjT"])
@pytest.mark.parametrize("N", [5, 40, 130])
def test_sums_and_aggregate_on_dirty_memory(env, transposed, N):
    n = 300
    src, dst = _graph(n)
    A = am.dense_view(src, dst, n, transposed)
    rng = np.random.default_rng(5)
    T = _x((n, N), 5)
    Q = rng.integers(0, 256, size=(n, N)).astype(np.uint8)      # contiguous: off the 4-byte rule for N = 5 and 130, so copied
    R, S = rng.random(n) < 0.5, rng.random(n) < 0.5
    d = [_up(env, a) for a in (src, dst, T, nm.bitmap(R), nm.bitmap(S), Q)]

    def run():
        adj = env.Q.pack_edges_tiled(d[0], d[1], n)            # packed on dirty memory too
        a = adj.T if transposed else adj
        return [env.af.tiledMMCodes(a, d[5]), env.af.tiledMMCodes(a, d[5], d[3], d[4]), env.af.aggregate(a, d[2], 8, route="bytes"),
                env.af.aggregate(a, d[2], 2, a.mean_scale(row_mask=d[3], nbr_mask=d[4]), d[3], d[4], route="bytes")]

    mean = am.inv_degree(am.masked_view(A, R, S).sum(axis=1))
    run()
    _under_both_patterns(env, f"bytes route transposed={transposed} N={N}", d, run,
                         [cm.tiled_mm_codes(A, Q), cm.tiled_mm_codes(A, Q, R, S), cm.aggregate(A, T, 8), cm.aggregate(A, T, 2, mean, R, S)])


@pytest.mark.parametrize("norm", [None, "sym"])
def test_the_layer_on_dirty_memory(env, norm):
    torch = env.torch
    n, dims = 300, (12, 20, 7)
    src, dst = _graph(n)
    A = am.dense_view(src, dst, n)
    rng = np.random.default_rng(6)
    X, W_in, W_out = (rng.normal(size=s).astype(F32) for s in ((n, dims[0]), (dims[0], dims[1]), (dims[1], dims[2])))
    nodes = rng.random(n) < 0.6
    layer = env.af.GCNConv_Affine(*dims, w_bit=4, act_bit=8, norm=norm, route="bytes").to(env.dev)
    with torch.no_grad():
        layer.W_in.copy_(_up(env, W_in))
        layer.W_out.copy_(_up(env, W_out))
    d = [_up(env, a) for a in (src, dst, X, nodes)]

    def run():
        adj = env.Q.pack_edges_tiled(d[0], d[1], n, reorder=True)
        return [layer(adj, d[2]), layer(adj, d[2], nodes=d[3])]

    run()
    _under_both_patterns(env, f"GCNConv_Affine route=bytes norm={norm}", d + [layer.W_in, layer.W_out], run,
                         [am.gcn(A, X, W_in, W_out, 4, 8, norm), am.gcn(A, X, W_in, W_out, 4, 8, norm, nodes)])
