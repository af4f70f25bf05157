"""The edge-value entries off the default stream and under graph capture: the ctypes entries (qgtc_tiled_value_index,
qgtc_tiled_edge_slots, qgtc_tiled_edge_endpoints, qgtc_tiled_sddmm_f32) take the handle of torch's current stream and the weighted
products run on current_stream(X), so behind a head start of plain torch work on a side stream they see operands a producer wrote on
that stream, and a captured graph replays them on new contents of `values`. The machine's GPU_MAX_HW_QUEUES is left alone."""
import numpy as np
import pytest

import tiled_edge_model as em
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

    n, N = 300, 40
    rng = np.random.default_rng(5)
    src, dst = (np.asarray(a, dtype=np.int64) for a in random_edges(rng, n, 6 * n))
    adj = QGTC.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    adj.T   # the column index, before any capture
    row, col = em.slot_cells(src, dst, n)
    data = [(rng.normal(size=row.size).astype(np.float32), rng.normal(size=(n, N)).astype(np.float32),
             rng.normal(size=(n, N)).astype(np.float32)) for _ in range(3)]   # (values, X, dY)
    return torch, QGTC, n, src, dst, adj, row, col, data


def _head_start(torch):
    a, b = torch.rand(2048, 2048, device="cuda"), torch.rand(2048, 2048, device="cuda")
    for _ in range(8):
        a = torch.mm(a, b).clamp_(0, 1)   # work queued ahead on the current (side) stream
    return a


def test_index_entries_follow_the_current_stream(setup):
    torch, QGTC, n, src, dst, adj, row, col, data = setup
    from qgtc_ppopp22_amd import tiled

    want_ptr, want_row = em.value_index(src, dst, n)
    pinned_tiles = adj.tiles.cpu().pin_memory()
    pinned_src, pinned_dst = torch.from_numpy(row).pin_memory(), torch.from_numpy(col).pin_memory()
    tiles = torch.zeros_like(adj.tiles)
    es, ed = torch.zeros(row.size, dtype=torch.int64, device="cuda"), torch.zeros(row.size, dtype=torch.int64, device="cuda")
    tiled._value_index(adj)   # the shared adjacency's index, before the side stream
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _head_start(torch)
        tiles.copy_(pinned_tiles, non_blocking=True)   # the producer: the tiles arrive on this stream
        es.copy_(pinned_src, non_blocking=True)
        ed.copy_(pinned_dst, non_blocking=True)
        fresh = QGTC.TiledAdjacency(n, adj.row_ptr, adj.kquad, tiles)
        val_ptr, val_row, nnz = tiled._value_index(fresh)   # a launch on another stream would have counted zero tiles
        r, c = tiled.edge_endpoints(fresh)
        slots = tiled.edge_slots(adj, es, ed)               # ... or looked up the edges (0, 0)
    side.synchronize()
    assert nnz == row.size and np.array_equal(val_ptr.cpu().numpy(), want_ptr) and np.array_equal(val_row.cpu().numpy(), want_row)
    assert np.array_equal(r.cpu().numpy(), row) and np.array_equal(c.cpu().numpy(), col)
    assert torch.equal(slots.cpu(), torch.arange(row.size))
    torch.cuda.current_stream().wait_stream(side)


@pytest.mark.parametrize("transposed", [False, True])
def test_weighted_launch_and_sddmm_on_a_side_stream_and_under_capture(setup, transposed):
    torch, QGTC, n, src, dst, adj, row, col, data = setup
    from qgtc_ppopp22_amd import tiled

    a = adj.T if transposed else adj
    pinned = [tuple(torch.from_numpy(t).pin_memory() for t in d) for d in data]
    v, X, dY = (torch.zeros_like(_dev(torch, t)) for t in data[0])

    def run():
        Xg, vg = X.clone().requires_grad_(True), v.clone().requires_grad_(True)
        Y = QGTC.tiledAggregate(a, Xg, edge_weight=vg)
        gX, gv = torch.autograd.grad(Y, (Xg, vg), dY)
        return [Y.detach(), gX, gv, tiled.tiledSDDMM(a, dY, X)]

    def want(d):
        vals, Xn, dYn = d
        return [em.weighted_f32(src, dst, n, Xn, vals, transposed), em.weighted_f32(src, dst, n, dYn, vals, not transposed),
                em.sddmm_f32(src, dst, n, dYn, Xn, transposed), em.sddmm_f32(src, dst, n, dYn, Xn, transposed)]

    def check(got, d, what):
        for k, (g, w) in enumerate(zip(got, want(d))):
            assert _same(g, w), (what, k)

    for t, p in zip((v, X, dY), pinned[0]):
        t.copy_(p)
    check(run(), data[0], "eager")   # the warm-up: the index and the column index exist from here on
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _head_start(torch)
        for t, p in zip((v, X, dY), pinned[1]):
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
        for t, p in zip((v, X, dY), pinned[k]):
            t.copy_(p)
        graph.replay()
        torch.cuda.synchronize()
        check(got, data[k], f"replay {k}")
