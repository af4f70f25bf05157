"""The byte-code route off the default stream and under graph capture (include/qgtc_codes.h): the five C entries are reached through
ctypes with the handle of torch's current stream, so they must follow it, and the quantisation parameters are computed and read on the
device, so a replay must follow the RANGE of the data as well as its values. One ``Live`` case of tests/stream_cases.py for the
primitives (qparams -> codes -> tiledMMCodes), one for ``affine.aggregate(route="bytes")`` per view, plain and masked, and one for the
layer: ``ordering_probe`` puts them behind a timed head start on fresh side streams, ``capture_and_replay`` replays them on three new
contents. The four contents of every case are the four ranges of tests/test_affine_streams_gpu.py, so each has its own scale and zero
point. All checks are bit for bit against tests/tiled_codes_model.py and tests/affine_model.py."""
import numpy as np
import pytest

import affine_model as am
import tiled_codes_model as cm
import tiled_nodes_model as nm
from stream_cases import Live, capture_and_replay, empty, env_of, ordering_probe, warm_adjacency
from test_affine_streams_gpu import RANGES, _content
from tiled_model import random_edges

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def setup(qgtc, oracle):
    import torch

    env = env_of(qgtc, oracle, torch)
    n = 300
    src, dst = (np.asarray(a, dtype=np.int64) for a in random_edges(np.random.default_rng(61), n, 3 * n))
    adj = warm_adjacency(env, src, dst, n)
    return env, n, src, dst, adj


def _primitives_live(env, n, src, dst, adj):
    """T [n, N] -> its parameters, its byte codes (the whole buffer, pad bytes included) and their neighbour sums on both views"""
    from qgtc_ppopp22_amd import affine

    torch = env.torch
    N, bits = 37, 8
    A, At = am.dense_view(src, dst, n), am.dense_view(src, dst, n, True)
    rng = np.random.default_rng(66)
    contents, wants = [], []
    for k in range(len(RANGES)):
        T = _content(rng, (n, N), k)
        qt = am.qparams(T, bits)
        Q = cm.codes(T, qt, bits)
        wants.append([qt, cm.codes_buffer(T, qt, bits), cm.tiled_mm_codes(A, Q), cm.tiled_mm_codes(At, Q)])
        contents.append([T])
    T = empty(env, (n, N), torch.float32)

    def run():
        qt = affine.qparams(T, bits)
        Q = affine.codes(T, bits, qt)
        return [qt, Q.as_strided((n, cm.pad4(N)), (cm.pad4(N), 1)), affine.tiledMMCodes(adj, Q), affine.tiledMMCodes(adj.T, Q)]

    return Live(torch, [T], contents, wants, run=run, keep=adj)


def test_the_primitives_on_a_side_stream_and_under_capture(setup):
    env = setup[0]
    live = _primitives_live(env, *setup[1:])
    ordering_probe(env.torch, env.Q, live, "codes primitives")
    capture_and_replay(env.torch, env.Q, live, "codes primitives")


def _aggregate_live(env, transposed, n, src, dst, adj):
    from qgtc_ppopp22_amd import affine

    torch = env.torch
    N = 40
    a = adj.T if transposed else adj
    A = am.dense_view(src, dst, n, transposed)
    rng = np.random.default_rng(67 + transposed)
    contents, wants = [], []
    for k in range(len(RANGES)):
        T = _content(rng, (n, N), k)
        R, S = rng.random(n) < 0.5, rng.random(n) < 0.5
        mean = am.inv_degree(am.masked_view(A, R, S).sum(axis=1))
        wants.append([cm.aggregate(A, T, 8), cm.aggregate(A, T, 4, mean, R, S)])
        contents.append([T, nm.bitmap(R), nm.bitmap(S)])
    T = empty(env, (n, N), torch.float32)
    rm, sm = empty(env, (adj.mask_words,), torch.int32), empty(env, (adj.mask_words,), torch.int32)

    def run():
        return [affine.aggregate(a, T, 8, route="bytes"),
                affine.aggregate(a, T, 4, a.mean_scale(row_mask=rm, nbr_mask=sm), row_mask=rm, nbr_mask=sm, route="bytes")]

    return Live(torch, [T, rm, sm], contents, wants, run=run, keep=adj)


@pytest.mark.parametrize("transposed", [False, True], ids=["adj", "adjT"])
def test_aggregate_on_a_side_stream_and_under_capture(setup, transposed):
    env = setup[0]
    live = _aggregate_live(env, transposed, *setup[1:])
    what = f"affine.aggregate(route='bytes'), {'adj.T' if transposed else 'adj'}"
    ordering_probe(env.torch, env.Q, live, what)
    capture_and_replay(env.torch, env.Q, live, what)


def _layer_live(env, n, src, dst, adj):
    from qgtc_ppopp22_amd import affine

    torch = env.torch
    F_in, H, C = 12, 20, 7
    A = am.dense_view(src, dst, n)
    rng = np.random.default_rng(69)
    W_in, W_out = rng.normal(size=(F_in, H)).astype(F32), rng.normal(size=(H, C)).astype(F32)
    layer = affine.GCNConv_Affine(F_in, H, C, w_bit=4, act_bit=8, norm="mean", route="bytes").to(env.dev)
    with torch.no_grad():
        layer.W_in.copy_(torch.from_numpy(W_in))
        layer.W_out.copy_(torch.from_numpy(W_out))
    contents, wants = [], []
    for k in range(len(RANGES)):
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
    ordering_probe(env.torch, env.Q, live, "GCNConv_Affine(route='bytes')")
    capture_and_replay(env.torch, env.Q, live, "GCNConv_Affine(route='bytes')")
