"""The edge softmax off the default stream and under graph capture: the ctypes entries (qgtc_tiled_edge_softmax_f32 / _t and their
gradients) take the handle of torch's current stream. One ``Live`` case of tests/stream_cases.py per view: ``ordering_probe`` puts the
softmax, its gradient and the whole attention behind a timed head start on three fresh side streams, where they must see logits a
producer wrote on that stream, and ``capture_and_replay`` replays them on three new contents of the operands. The checks are bit for bit
against tests/tiled_esoftmax_model.py. The machine's GPU_MAX_HW_QUEUES is left alone."""
import numpy as np
import pytest

import tiled_edge_model as em
import tiled_esoftmax_model as sm
from stream_cases import Live, capture_and_replay, empty, env_of, ordering_probe, warm_adjacency
from tiled_model import random_edges

pytestmark = pytest.mark.gpu


def _live(env, transposed):
    from qgtc_ppopp22_amd import tiled

    torch = env.torch
    n, d, N = 300, 24, 40
    rng = np.random.default_rng(5)
    src, dst = (np.asarray(a, dtype=np.int64) for a in random_edges(rng, n, 6 * n))
    adj = warm_adjacency(env, src, dst, n)
    a = adj.T if transposed else adj
    nnz = em.slot_cells(src, dst, n)[0].size
    data = [((3 * rng.normal(size=nnz)).astype(np.float32), rng.normal(size=nnz).astype(np.float32),
             rng.normal(size=(n, d)).astype(np.float32), rng.normal(size=(n, d)).astype(np.float32),
             rng.normal(size=(n, N)).astype(np.float32), rng.normal(size=(n, N)).astype(np.float32))
            for _ in range(4)]   # (logits, g, Q, K, V, dY)
    L, g, Q, K, V, dY = bufs = [empty(env, t.shape, torch.float32) for t in data[0]]

    def run():
        Lg = L.clone().requires_grad_(True)
        alpha, m, inv = tiled.tiledEdgeSoftmax(a, Lg, return_stats=True)
        gl, = torch.autograd.grad(alpha, Lg, g)
        Qg, Kg, Vg = (t.clone().requires_grad_(True) for t in (Q, K, V))
        Y = tiled.tiledEdgeAttention(a, Qg, Kg, Vg, scale=0.25)
        gQ, gK, gV = torch.autograd.grad(Y, (Qg, Kg, Vg), dY)
        return [alpha.detach(), m, inv, gl, Y.detach(), gQ, gK, gV]

    def want(c):
        ln, gn, Qn, Kn, Vn, dYn = c
        alpha, m, inv = sm.edge_softmax_f32(src, dst, n, ln, transposed)
        return [alpha, m, inv, sm.edge_softmax_grad_f32(src, dst, n, alpha, gn, transposed),
                sm.edge_attention_f32(src, dst, n, Qn, Kn, Vn, 0.25, transposed)[0],
                *sm.edge_attention_grads_f32(src, dst, n, Qn, Kn, Vn, 0.25, dYn, transposed)]

    return Live(torch, bufs, data, [[np.asarray(w, dtype=np.float32) for w in want(c)] for c in data], run=run, keep=adj)


@pytest.mark.parametrize("transposed", [False, True])
def test_softmax_and_attention_on_a_side_stream_and_under_capture(qgtc, oracle, transposed):
    import torch

    live = _live(env_of(qgtc, oracle, torch), transposed)
    what = f"edge softmax and attention, {'adj.T' if transposed else 'adj'}"
    ordering_probe(torch, qgtc, live, what)
    capture_and_replay(torch, qgtc, live, what)
