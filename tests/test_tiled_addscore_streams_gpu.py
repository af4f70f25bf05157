"""The additive-score entries off the default stream and under graph capture (include/qgtc_addscore.h: the score and its gradient folds
on both views): each ctypes entry takes the handle of torch's current stream, so behind a head start of plain torch work on a side
stream it sees operands a producer wrote on that stream, and a captured graph replays every entry - alone and composed into the GATv2
attention with its four gradients - on new contents of the operands. The checks are bit for bit against the model of
tests/tiled_addscore_model.py. The machine's GPU_MAX_HW_QUEUES is left alone."""
import numpy as np
import pytest

import tiled_addscore_model as am
import tiled_edge_model as em
from tiled_model import random_edges

pytestmark = pytest.mark.gpu

H, D, DV = 4, 6, 10   # own and nbr are [n, 24], V is [n, 40]
SLOPE = 0.2


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
    rng = np.random.default_rng(6)
    src, dst = (np.asarray(a, dtype=np.int64) for a in random_edges(rng, n, 6 * n))
    adj = QGTC.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    adj.T   # the column index, before any capture
    nnz = em.slot_cells(src, dst, n)[0].size
    data = [(rng.normal(size=(nnz, H)).astype(np.float32), rng.normal(size=(n, H * D)).astype(np.float32),
             rng.normal(size=(n, H * D)).astype(np.float32), rng.normal(size=(H, D)).astype(np.float32),
             rng.normal(size=(n, H * DV)).astype(np.float32), rng.normal(size=(n, H * DV)).astype(np.float32))
            for _ in range(3)]   # (g, own, nbr, att, V, dY)
    return torch, n, src, dst, adj, data


def _head_start(torch):
    a, b = torch.rand(2048, 2048, device="cuda"), torch.rand(2048, 2048, device="cuda")
    for _ in range(8):
        a = torch.mm(a, b).clamp_(0, 1)   # work queued ahead on the current (side) stream
    return a


@pytest.mark.parametrize("transposed", [False, True])
def test_every_entry_on_a_side_stream_and_under_capture(setup, transposed):
    torch, n, src, dst, adj, data = setup
    from qgtc_ppopp22_amd import tiled

    a = adj.T if transposed else adj
    pinned = [tuple(torch.from_numpy(t).pin_memory() for t in d) for d in data]
    bufs = tuple(torch.zeros_like(_dev(torch, t)) for t in data[0])
    g, own, nbr, att, V, dY = bufs

    def run():
        s = tiled.tiledEdgeAdditiveScores(a, own, nbr, att, SLOPE, heads=H)           # the score entry
        d_own, P = tiled._addscore_grad(a, own, nbr, att, SLOPE, g, H, True, True)     # the gradient entry of this view, both outputs
        d_nbr, _ = tiled._addscore_grad(a.T, nbr, own, att, SLOPE, g, H, True, False)  # and of the other, one output
        leaves = [t.clone().requires_grad_(True) for t in (own, nbr, V, att)]
        Y = tiled.tiledEdgeAdditiveAttention(a, leaves[0], leaves[1], leaves[2], leaves[3], SLOPE, heads=H)
        go, gn, gV, ga = torch.autograd.grad(Y, leaves, dY)
        return [s, d_own, P, d_nbr, Y.detach(), go, gn, gV, ga]

    def want(d):
        gn, on, nn, an, Vn, dYn = d
        d_own, P = am.addscore_grad_heads_f32(src, dst, n, on, nn, an, SLOPE, gn, H, transposed)
        d_nbr, _ = am.addscore_grad_heads_f32(src, dst, n, nn, on, an, SLOPE, gn, H, not transposed)
        w_own, w_nbr, w_V, w_P = am.additive_attention_grads_heads_f32(src, dst, n, on, nn, Vn, an, SLOPE, H, dYn, transposed)
        return [am.addscore_heads_f32(src, dst, n, on, nn, an, SLOPE, H, transposed), d_own, P, d_nbr,
                am.additive_attention_heads_f32(src, dst, n, on, nn, Vn, an, SLOPE, H, transposed)[0], w_own, w_nbr, w_V,
                _dev(torch, w_P).sum(dim=0).view(H, D).cpu().numpy()]   # att's gradient: torch's reduction of the model's P

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
