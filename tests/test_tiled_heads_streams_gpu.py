"""The multi-head entries off the default stream and under graph capture (include/qgtc_heads.h: the per-edge dot, the weighted sum on
both views, the edge softmax and its gradient on both views): each ctypes entry takes the handle of torch's current stream. One ``Live``
case of tests/stream_cases.py per view: ``ordering_probe`` puts every entry - alone and composed into the attention with heads and its
three gradients - behind a timed head start on three fresh side streams, where it must see operands a producer wrote on that stream, and
``capture_and_replay`` replays them on three new contents of the operands. The checks are bit for bit against the per-head models. The
machine's GPU_MAX_HW_QUEUES is left alone."""
import numpy as np
import pytest

import tiled_edge_model as em
import tiled_heads_model as hm
from stream_cases import Live, capture_and_replay, empty, env_of, ordering_probe, warm_adjacency
from tiled_model import random_edges

pytestmark = pytest.mark.gpu

H, D, DV = 4, 6, 10   # Q and K are [n, 24], V is [n, 40]


def _live(env, transposed):
    from qgtc_ppopp22_amd import tiled

    torch, QGTC = env.torch, env.Q
    n = 300
    rng = np.random.default_rng(5)
    src, dst = (np.asarray(a, dtype=np.int64) for a in random_edges(rng, n, 6 * n))
    adj = warm_adjacency(env, src, dst, n)
    a = adj.T if transposed else adj
    nnz = em.slot_cells(src, dst, n)[0].size
    data = [((3 * rng.normal(size=(nnz, H))).astype(np.float32), rng.normal(size=(nnz, H)).astype(np.float32),
             rng.normal(size=(n, H * D)).astype(np.float32), rng.normal(size=(n, H * D)).astype(np.float32),
             rng.normal(size=(n, H * DV)).astype(np.float32), rng.normal(size=(n, H * DV)).astype(np.float32))
            for _ in range(4)]   # (logits, g, Q, K, V, dY)
    L, g, Q, K, V, dY = bufs = [empty(env, t.shape, torch.float32) for t in data[0]]

    def run():
        Lg = L.clone().requires_grad_(True)
        alpha, m, inv = tiled.tiledEdgeSoftmax(a, Lg, return_stats=True)   # the softmax entry of this view
        gl, = torch.autograd.grad(alpha, Lg, g)                             # its gradient entry
        s = tiled.tiledSDDMM(a, Q, K, heads=H)                              # the per-edge dot
        W = QGTC.tiledMMFloat(a, V, edge_weight=g)                          # the weighted sum of this view
        Wt = QGTC.tiledMMFloat(a.T, V, edge_weight=g)                       # and of the other
        Qg, Kg, Vg = (t.clone().requires_grad_(True) for t in (Q, K, V))
        Y = tiled.tiledEdgeAttention(a, Qg, Kg, Vg, scale=0.25, heads=H)
        gQ, gK, gV = torch.autograd.grad(Y, (Qg, Kg, Vg), dY)
        return [alpha.detach(), m, inv, gl, s, W, Wt, Y.detach(), gQ, gK, gV]

    def want(c):
        ln, gn, Qn, Kn, Vn, dYn = c
        alpha, m, inv = hm.edge_softmax_heads_f32(src, dst, n, ln, transposed)
        return [alpha, m, inv, hm.edge_softmax_grad_heads_f32(src, dst, n, alpha, gn, transposed),
                hm.sddmm_heads_f32(src, dst, n, Qn, Kn, H, transposed), hm.weighted_heads_f32(src, dst, n, Vn, gn, transposed),
                hm.weighted_heads_f32(src, dst, n, Vn, gn, not transposed),
                hm.edge_attention_heads_f32(src, dst, n, Qn, Kn, Vn, H, 0.25, transposed),
                *hm.edge_attention_grads_heads_f32(src, dst, n, Qn, Kn, Vn, H, dYn, 0.25, transposed)]

    return Live(torch, bufs, data, [[np.asarray(w, dtype=np.float32) for w in want(c)] for c in data], run=run, keep=adj)


@pytest.mark.parametrize("transposed", [False, True])
def test_every_entry_on_a_side_stream_and_under_capture(qgtc, oracle, transposed):
    import torch

    live = _live(env_of(qgtc, oracle, torch), transposed)
    what = f"the entries with heads, {'adj.T' if transposed else 'adj'}"
    ordering_probe(torch, qgtc, live, what)
    capture_and_replay(torch, qgtc, live, what)
