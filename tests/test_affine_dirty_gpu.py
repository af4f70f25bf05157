"""Affine quantisation on recycled, poisoned device memory (tests/dirty_memory.py; DESIGN.md, "Dirty memory"): every output of
qgtc_ppopp22_amd/affine.py comes from ``torch.empty`` - the parameter table, the packed words with their pad words, the code sums, the
dequantised matrix - and so does the scratch of the range launch, which is handed to the entry holding the poison and never cleared. Each
primitive, ``linear``, ``aggregate`` and the layer run under ``dirty`` once per pattern; every word must equal tests/affine_model.py bit
for bit, and the two patterns' results each other."""
import numpy as np
import pytest

import affine_model as am
import dirty_memory as dm
import stream_cases as sc
import tiled_nodes_model as nm
from tiled_model import random_edges

pytestmark = pytest.mark.gpu
F32 = np.float32
MODULE = "tests/test_affine_dirty_gpu.py"


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


@pytest.mark.parametrize("shape", [(33, 130), (70, 131), (257, 64)], ids=str)      # (70, 131): three workgroups of partials in `work`
def test_qparams_on_dirty_memory(env, shape):
    x = _x(shape, 1)
    dx = _up(env, x)
    for bits in (2, 8):
        _under_both_patterns(env, f"qparams {shape} {bits} bits", [dx],
                             lambda: [env.af.qparams(dx, bits), env.af.qparams(dx, bits, per_column=True)],
                             [am.qparams(x, bits), am.qparams(x, bits, True)])


@pytest.mark.parametrize("col_major", [False, True], ids=["rows", "cols"])
@pytest.mark.parametrize("shape", [(33, 130), (37, 256), (100, 260)], ids=str)
def test_val2bit_affine_on_dirty_memory(env, shape, col_major):
    x = _x(shape, 2)
    dx = _up(env, x)
    for bits in (3, 8):
        want, d_qp = [], []
        for per_column in (False, True):
            qp = am.qparams(x, bits, per_column)
            q = am.quantise(x, qp, bits)
            want += [env.O.pack(q, bits, col_major, False).view(np.int32), am.sums(q, col_major)]
            d_qp.append(_up(env, qp))

        def run():
            out = []
            for qp in d_qp:
                words, sums = env.af.val2bit_affine(dx, bits, qp, col_major)
                out += [words.reshape(-1), sums]
            return out

        _under_both_patterns(env, f"val2bit_affine {shape} {bits} bits col_major={col_major}", [dx] + d_qp, run, want)


def test_dequant_on_dirty_memory(env):
    rng = np.random.default_rng(3)
    M, N, K = 100, 64, 77
    acc = rng.integers(0, 2 ** 22, size=(M, N)).astype(F32)
    qa = np.array([[0.02, 7, 50, 0]], F32)
    qb = np.stack([rng.random(N).astype(F32) + F32(0.01), rng.integers(0, 16, N).astype(F32), np.ones(N, F32), np.zeros(N, F32)], axis=1)
    rs, cs = rng.integers(0, 255 * K, M).astype(np.int32), rng.integers(0, 15 * K, N).astype(np.int32)
    scale, bias = rng.normal(size=M).astype(F32), rng.normal(size=N).astype(F32)
    d = [_up(env, a) for a in (acc, qa, rs, qb, cs, scale, bias)]
    _under_both_patterns(env, "dequant", d,
                         lambda: [env.af.dequant(d[0], K, d[1], d[2], d[3], d[4]), env.af.dequant(d[0], K, d[1], None, d[3], None, d[5], d[6], True)],
                         [am.dequant(acc, K, qa, rs, qb, cs), am.dequant(acc, K, qa, None, qb, None, scale, bias, True)])


def test_linear_on_dirty_memory(env):
    rng = np.random.default_rng(4)
    X, W = _x((100, 130), 4), (rng.normal(size=(130, 64)) * 2.0 ** rng.integers(-3, 4, size=(1, 64))).astype(F32)
    dX, dW = _up(env, X), _up(env, W)
    _under_both_patterns(env, "linear", [dX, dW], lambda: [env.af.linear(dX, dW, 8, 4), env.af.linear(dX, dW, 4, 2, False)],
                         [am.linear(X, W, 8, 4), am.linear(X, W, 4, 2, False)])


def _graph(n):
    return tuple(np.asarray(a, dtype=np.int64) for a in random_edges(np.random.default_rng(70 + n), n, 3 * n))


@pytest.mark.parametrize("transposed", [False, True], ids=["adj", "adjT"])
def test_aggregate_on_dirty_memory(env, transposed):
    n, N = 300, 40
    src, dst = _graph(n)
    A = am.dense_view(src, dst, n, transposed)
    rng = np.random.default_rng(5)
    T = _x((n, N), 5)
    R, S = rng.random(n) < 0.5, rng.random(n) < 0.5
    d = [_up(env, a) for a in (src, dst, T, nm.bitmap(R), nm.bitmap(S))]

    def run():
        adj = env.Q.pack_edges_tiled(d[0], d[1], n)            # packed on dirty memory too
        a = adj.T if transposed else adj
        return [env.af.aggregate(a, d[2], 8), env.af.aggregate(a, d[2], 2, a.mean_scale(row_mask=d[3], nbr_mask=d[4]), d[3], d[4])]

    mean = am.inv_degree(am.masked_view(A, R, S).sum(axis=1))
    _under_both_patterns(env, f"aggregate transposed={transposed}", d, run, [am.aggregate(A, T, 8), am.aggregate(A, T, 2, mean, R, S)])


@pytest.mark.parametrize("norm", [None, "sym"])
def test_the_layer_on_dirty_memory(env, norm):
    torch = env.torch
    n, dims = 300, (12, 20, 7)
    src, dst = _graph(n)
    A = am.dense_view(src, dst, n)
    rng = np.random.default_rng(6)
    X, W_in, W_out = (rng.normal(size=s).astype(F32) for s in ((n, dims[0]), (dims[0], dims[1]), (dims[1], dims[2])))
    nodes = rng.random(n) < 0.6
    layer = env.af.GCNConv_Affine(*dims, w_bit=4, act_bit=8, norm=norm).to(env.dev)
    with torch.no_grad():
        layer.W_in.copy_(_up(env, W_in))
        layer.W_out.copy_(_up(env, W_out))
    d = [_up(env, a) for a in (src, dst, X, nodes)]

    def run():
        adj = env.Q.pack_edges_tiled(d[0], d[1], n, reorder=True)
        return [layer(adj, d[2]), layer(adj, d[2], nodes=d[3])]

    _under_both_patterns(env, f"GCNConv_Affine norm={norm}", d + [layer.W_in, layer.W_out], run,
                         [am.gcn(A, X, W_in, W_out, 4, 8, norm), am.gcn(A, X, W_in, W_out, 4, 8, norm, nodes)])
