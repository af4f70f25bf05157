"""The multi-head entries off the default stream and under graph capture (include/qgtc_heads.h: the per-edge dot, the weighted sum on
both views, the edge softmax and its gradient on both views): each ctypes entry takes the handle of torch's current stream, so behind
a head start of plain torch work on a side stream it sees operands a producer wrote on that stream, and a captured graph replays every
entry - alone and composed into the attention with heads and its three gradients - on new contents of the operands. The checks are
bit for bit against the per-head models. The machine's GPU_MAX_HW_QUEUES is left alone."""
import numpy as np
import pytest

import tiled_edge_model as em
import tiled_heads_model as hm
from tiled_model import random_edges

pytestmark = pytest.mark.gpu

H, D, DV = 4, 6, 10   # Q and K are [n, 24], V is [n, 40]


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(got, want):
    return np.array_equal(got.detach().cpu().numpy().view(np.uint32), np.ascontiguousarray(want, dtype=np.float32).view(np.uint32))


@pytest.fixture(scope="module")
def setup():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import QGTC

    n = 300
    rng = np.random.default_rng(5)
    src, dst = (np.asarray(a, dtype=np.int64) for a in random_edges(rng, n, 6 * n))
    adj = QGTC.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    adj.T   # the column index, before any capture
    nnz = em.slot_cells(src, dst, n)[0].size
    data = [((3 * rng.normal(size=(nnz, H))).astype(np.float32), rng.normal(size=(nnz, H)).astype(np.float32),
             rng.normal(size=(n, H * D)).astype(np.float32), rng.normal(size=(n, H * D)).astype(np.float32),
             rng.normal(size=(n, H * DV)).astype(np.float32), rng.normal(size=(n, H * DV)).astype(np.float32))
            for _ in range(3)]   # (logits, g, Q, K, V, dY)
    return torch, n, src, dst, adj, data


def _head_start(torch):
    a, b = torch.rand(2048, 2048, device="cuda"), torch.rand(2048, 2048, device="cuda")
    for _ in range(8):
        a = torch.mm(a, b).clamp_(0, 1)   # work queued ahead on the current (side) stream
    return a


@pytest.mark.parametrize("transposed", [False, True])
def test_every_entry_on_a_side_stream_and_under_capture(setup, transposed):
    torch, n, src, dst, adj, data = setup
    import QGTC
    from qgtc_ppopp22_amd import tiled

    a = adj.T if transposed else adj
    pinned = [tuple(torch.from_numpy(t).pin_memory() for t in d) for d in data]
    bufs = tuple(torch.zeros_like(_dev(torch, t)) for t in data[0])
    L, g, Q, K, V, dY = bufs

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

    def want(d):
        ln, gn, Qn, Kn, Vn, dYn = d
        alpha, m, inv = hm.edge_softmax_heads_f32(src, dst, n, ln, transposed)
        return [alpha, m, inv, hm.edge_softmax_grad_heads_f32(src, dst, n, alpha, gn, transposed),
                hm.sddmm_heads_f32(src, dst, n, Qn, Kn, H, transposed), hm.weighted_heads_f32(src, dst, n, Vn, gn, transposed),
                hm.weighted_heads_f32(src, dst, n, Vn, gn, not transposed),
                hm.edge_attention_heads_f32(src, dst, n, Qn, Kn, Vn, H, 0.25, transposed),
                *hm.edge_attention_grads_heads_f32(src, dst, n, Qn, Kn, Vn, H, dYn, 0.25, transposed)]

    wants = [want(d) for d in data]

    def check(got, k, what):
        for i, (x, w) in enumerate(zip(got, wants[k])):
            assert _same(x, w), (what, i)

    for t, p in zip(bufs, pinned[0]):
        t.copy_(p)
    check(run(), 0, "eager")   # the warm-up: the index and the column index exist from here on
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _head_start(torch)
        for t, p in zip(bufs, pinned[1]):
            t.copy_(p, non_blocking=True)   # the pending producer on this stream
        got = run()
    side.synchronize()
    check(got, 1, "side stream: a launch on another stream would have read the previous operands")
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = run()
    for k in (2, 0):
        for t, p in zip(bufs, pinned[k]):
            t.copy_(p)
        graph.replay()
        torch.cuda.synchronize()
        check(got, k, f"replay {k}")
