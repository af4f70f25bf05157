"""The edge softmax off the default stream and under graph capture: the ctypes entries (qgtc_tiled_edge_softmax_f32 / _t and their
gradients) take the handle of torch's current stream, so behind a head start of plain torch work on a side stream they see logits a
producer wrote on that stream, and a captured graph replays the softmax, its gradient and the whole attention on new contents of the
operands. The machine's GPU_MAX_HW_QUEUES is left alone."""
import numpy as np
import pytest

import tiled_edge_model as em
import tiled_esoftmax_model as sm
from tiled_model import random_edges

pytestmark = pytest.mark.gpu


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

    n, d, N = 300, 24, 40
    rng = np.random.default_rng(5)
    src, dst = (np.asarray(a, dtype=np.int64) for a in random_edges(rng, n, 6 * n))
    adj = QGTC.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    adj.T   # the column index, before any capture
    nnz = em.slot_cells(src, dst, n)[0].size
    data = [((3 * rng.normal(size=nnz)).astype(np.float32), rng.normal(size=nnz).astype(np.float32),
             rng.normal(size=(n, d)).astype(np.float32), rng.normal(size=(n, d)).astype(np.float32),
             rng.normal(size=(n, N)).astype(np.float32), rng.normal(size=(n, N)).astype(np.float32))
            for _ in range(3)]   # (logits, g, Q, K, V, dY)
    return torch, n, src, dst, adj, data


def _head_start(torch):
    a, b = torch.rand(2048, 2048, device="cuda"), torch.rand(2048, 2048, device="cuda")
    for _ in range(8):
        a = torch.mm(a, b).clamp_(0, 1)   # work queued ahead on the current (side) stream
    return a


@pytest.mark.parametrize("transposed", [False, True])
def test_softmax_and_attention_on_a_side_stream_and_under_capture(setup, transposed):
    torch, n, src, dst, adj, data = setup
    from qgtc_ppopp22_amd import tiled

    a = adj.T if transposed else adj
    pinned = [tuple(torch.from_numpy(t).pin_memory() for t in d) for d in data]
    bufs = tuple(torch.zeros_like(_dev(torch, t)) for t in data[0])
    L, g, Q, K, V, dY = bufs

    def run():
        Lg = L.clone().requires_grad_(True)
        alpha, m, inv = tiled.tiledEdgeSoftmax(a, Lg, return_stats=True)
        gl, = torch.autograd.grad(alpha, Lg, g)
        Qg, Kg, Vg = (t.clone().requires_grad_(True) for t in (Q, K, V))
        Y = tiled.tiledEdgeAttention(a, Qg, Kg, Vg, scale=0.25)
        gQ, gK, gV = torch.autograd.grad(Y, (Qg, Kg, Vg), dY)
        return [alpha.detach(), m, inv, gl, Y.detach(), gQ, gK, gV]

    def want(d):
        ln, gn, Qn, Kn, Vn, dYn = d
        alpha, m, inv = sm.edge_softmax_f32(src, dst, n, ln, transposed)
        return [alpha, m, inv, sm.edge_softmax_grad_f32(src, dst, n, alpha, gn, transposed),
                sm.edge_attention_f32(src, dst, n, Qn, Kn, Vn, 0.25, transposed)[0],
                *sm.edge_attention_grads_f32(src, dst, n, Qn, Kn, Vn, 0.25, dYn, transposed)]

    def check(got, d, what):
        for k, (x, w) in enumerate(zip(got, want(d))):
            assert _same(x, w), (what, k)

    for t, p in zip(bufs, pinned[0]):
        t.copy_(p)
    check(run(), data[0], "eager")   # the warm-up: the index and the column index exist from here on
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _head_start(torch)
        for t, p in zip(bufs, pinned[1]):
            t.copy_(p, non_blocking=True)   # the pending producer on this stream
        got = run()
    side.synchronize()
    check(got, data[1], "side stream: a launch on another stream would have read the previous operands")
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
        check(got, data[k], f"replay {k}")
