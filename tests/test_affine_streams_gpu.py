"""Affine quantisation off the default stream and under graph capture (include/qgtc_affine.h): the four C entries are reached through
ctypes with the handle of torch's current stream, so they must follow it, and the quantisation parameters are computed and read on the
device, so a replay must follow the RANGE of the data as well as its values. One ``Live`` case of tests/stream_cases.py for the
primitives (qparams -> val2bit_affine -> dequant), one for ``affine.aggregate`` per view and one for the layer: ``ordering_probe`` puts
them behind a timed head start on three fresh side streams, ``capture_and_replay`` replays them on three new contents. The four contents of
every case differ in values, in scale (by powers of ten) and in offset, so each has its own scale and zero point. All checks are bit for
bit against tests/affine_model.py. The machine's GPU_MAX_HW_QUEUES is left alone."""
import numpy as np
import pytest

import affine_model as am
import tiled_nodes_model as nm
from stream_cases import Live, capture_and_replay, empty, env_of, ordering_probe, warm_adjacency
from tiled_model import random_edges

pytestmark = pytest.mark.gpu
F32 = np.float32
RANGES = ((1.0, 0.0), (10.0, 3.0), (0.1, -0.5), (100.0, 40.0))      # (scale, offset) of the four contents


@pytest.fixture(scope="module")
def setup(qgtc, oracle):
    import torch

    env = env_of(qgtc, oracle, torch)
    n = 300
    src, dst = (np.asarray(a, dtype=np.int64) for a in random_edges(np.random.default_rng(61), n, 3 * n))
    adj = warm_adjacency(env, src, dst, n)
    return env, n, src, dst, adj


def _content(rng, shape, k):
    s, o = RANGES[k]
    return (rng.normal(size=shape) * s + o).astype(F32)


def _primitives_live(env):
    """X [M, K] -> its per-tensor parameters, rows-layout words and row sums; its per-column parameters, cols-layout words and column sums;
    and dequant of an accumulator buffer under all of them"""
    from qgtc_ppopp22_amd import affine

    torch = env.torch
    M, K, bits, terms = 37, 40, 4, 9
    rng = np.random.default_rng(62)
    scale, bias = rng.normal(size=M).astype(F32), rng.normal(size=K).astype(F32)
    contents, wants = [], []
    for k in range(4):
        X = _content(rng, (M, K), k)
        acc = rng.integers(0, 2 ** 20, size=(M, K)).astype(F32)
        qa, qc = am.qparams(X, bits), am.qparams(X, bits, True)
        ca, cc = am.quantise(X, qa, bits), am.quantise(X, qc, bits)
        rs, cs = am.sums(ca, False), am.sums(cc, True)
        wants.append([qa, env.O.pack(ca, bits, False).view(np.int32), rs, qc, env.O.pack(cc, bits, True).view(np.int32), cs,
                      am.dequant(acc, terms, qa, rs, qc, cs, scale, bias, True)])
        contents.append([X, acc])
    X, acc = empty(env, (M, K), torch.float32), empty(env, (M, K), torch.float32)
    d_scale, d_bias = torch.from_numpy(scale).to(env.dev), torch.from_numpy(bias).to(env.dev)

    def run():
        qa, qc = affine.qparams(X, bits), affine.qparams(X, bits, per_column=True)
        wa, rs = affine.val2bit_affine(X, bits, qa)
        wc, cs = affine.val2bit_affine(X, bits, qc, col_major=True)
        return [qa, wa.reshape(-1), rs, qc, wc.reshape(-1), cs, affine.dequant(acc, terms, qa, rs, qc, cs, d_scale, d_bias, True)]

    return Live(torch, [X, acc], contents, wants, run=run, keep=(d_scale, d_bias))


def test_the_primitives_on_a_side_stream_and_under_capture(setup):
    env = setup[0]
    live = _primitives_live(env)
    ordering_probe(env.torch, env.Q, live, "affine primitives")
    capture_and_replay(env.torch, env.Q, live, "affine primitives")


def _aggregate_live(env, transposed, n, src, dst, adj):
    from qgtc_ppopp22_amd import affine

    torch = env.torch
    N = 40
    a = adj.T if transposed else adj
    A = am.dense_view(src, dst, n, transposed)
    rng = np.random.default_rng(63 + transposed)
    contents, wants = [], []
    for k in range(4):
        T = _content(rng, (n, N), k)
        R, S = rng.random(n) < 0.5, rng.random(n) < 0.5
        mean = am.inv_degree(am.masked_view(A, R, S).sum(axis=1))
        wants.append([am.aggregate(A, T, 8), am.aggregate(A, T, 4, mean, R, S)])
        contents.append([T, nm.bitmap(R), nm.bitmap(S)])
    T = empty(env, (n, N), torch.float32)
    rm, sm = empty(env, (adj.mask_words,), torch.int32), empty(env, (adj.mask_words,), torch.int32)

    def run():
        return [affine.aggregate(a, T, 8), affine.aggregate(a, T, 4, a.mean_scale(row_mask=rm, nbr_mask=sm), row_mask=rm, nbr_mask=sm)]

    return Live(torch, [T, rm, sm], contents, wants, run=run, keep=adj)


@pytest.mark.parametrize("transposed", [False, True], ids=["adj", "adjT"])
def test_aggregate_on_a_side_stream_and_under_capture(setup, transposed):
    env = setup[0]
    live = _aggregate_live(env, transposed, *setup[1:])
    what = f"affine.aggregate, {'adj.T' if transposed else 'adj'}"
    ordering_probe(env.torch, env.Q, live, what)
    capture_and_replay(env.torch, env.Q, live, what)


def _layer_live(env, n, src, dst, adj):
    from qgtc_ppopp22_amd import affine

    torch = env.torch
    F_in, H, C = 12, 20, 7
    A = am.dense_view(src, dst, n)
    rng = np.random.default_rng(65)
    W_in, W_out = rng.normal(size=(F_in, H)).astype(F32), rng.normal(size=(H, C)).astype(F32)
    layer = affine.GCNConv_Affine(F_in, H, C, w_bit=4, act_bit=8, norm="mean").to(env.dev)
    with torch.no_grad():
        layer.W_in.copy_(torch.from_numpy(W_in))
        layer.W_out.copy_(torch.from_numpy(W_out))
    contents, wants = [], []
    for k in range(4):
        X = _content(rng, (n, F_in), k)
        nodes = rng.random(n) < 0.5
        wants.append([am.gcn(A, X, W_in, W_out, 4, 8, "mean"), am.gcn(A, X, W_in, W_out, 4, 8, "mean", nodes)])
        contents.append([X, nodes])
    X, flags = empty(env, (n, F_in), torch.float32), empty(env, (n,), torch.bool)

    def run():
        return [layer(adj, X), layer(adj, X, nodes=flags)]

    return Live(torch, [X, flags], contents, wants, run=run, keep=(adj, layer))


def test_the_layer_on_a_side_stream_and_under_capture(setup):
    env = setup[0]
    live = _layer_live(env, *setup[1:])
    ordering_probe(env.torch, env.Q, live, "GCNConv_Affine")
    capture_and_replay(env.torch, env.Q, live, "GCNConv_Affine")
