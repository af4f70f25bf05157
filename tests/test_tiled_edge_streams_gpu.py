"""The edge-value entries off the default stream and under graph capture: the ctypes entries (qgtc_tiled_value_index,
qgtc_tiled_edge_slots, qgtc_tiled_edge_endpoints, qgtc_tiled_sddmm_f32) take the handle of torch's current stream and the weighted
products run on current_stream(X). The weighted aggregate, its two gradients and the SDDMM are a ``Live`` case of tests/stream_cases.py:
``ordering_probe`` puts them behind a timed head start on three fresh side streams, ``capture_and_replay`` replays them on three new
contents of `values`, X and dY. The index entries return nnz to the host and cannot be captured: they get the head start alone. The
machine's GPU_MAX_HW_QUEUES is left alone."""
import numpy as np
import pytest

import tiled_edge_model as em
from stream_cases import Live, capture_and_replay, empty, env_of, head_start, ordering_probe, until_sensitive, warm_adjacency
from tiled_model import random_edges

pytestmark = pytest.mark.gpu

N_NODES, N_COLS = 300, 40


def _case():
    """the graph, the cells of its slots and four contents (values, X, dY), all from one generator"""
    n = N_NODES
    rng = np.random.default_rng(5)
    src, dst = (np.asarray(a, dtype=np.int64) for a in random_edges(rng, n, 6 * n))
    row, col = em.slot_cells(src, dst, n)
    data = [(rng.normal(size=row.size).astype(np.float32), rng.normal(size=(n, N_COLS)).astype(np.float32),
             rng.normal(size=(n, N_COLS)).astype(np.float32)) for _ in range(4)]
    return src, dst, row, col, data


def test_index_entries_follow_the_current_stream(qgtc, oracle):
    """The tiles and an edge list arrive behind the head start: a launch on another stream would have counted zero tiles, or looked up
    the edges (0, 0). ``edge_slots`` is queued while the head start still runs; ``_value_index`` is queued right behind that check and
    then blocks on its host read, so ``edge_endpoints`` runs behind it as it always did."""
    import torch

    from qgtc_ppopp22_amd import tiled

    env = env_of(qgtc, oracle, torch)
    n = N_NODES
    src, dst, row, col, _ = _case()
    adj = warm_adjacency(env, src, dst, n)
    want_ptr, want_row = em.value_index(src, dst, n)
    pinned_tiles = adj.tiles.cpu().pin_memory()
    pinned_src, pinned_dst = torch.from_numpy(row).pin_memory(), torch.from_numpy(col).pin_memory()
    tiles = torch.zeros_like(adj.tiles)
    es, ed = empty(env, (row.size,), torch.int64), empty(env, (row.size,), torch.int64)
    tiled._value_index(adj)   # the shared adjacency's index, before the side stream

    def attempt(scale):
        for t in (tiles, es, ed):
            t.zero_()
        torch.cuda.synchronize(env.dev)
        with torch.cuda.stream(torch.cuda.Stream(env.dev)):
            ev = head_start(torch, env.dev, scale)
            tiles.copy_(pinned_tiles, non_blocking=True)   # the producer: the tiles arrive on this stream
            es.copy_(pinned_src, non_blocking=True)
            ed.copy_(pinned_dst, non_blocking=True)
            slots = tiled.edge_slots(adj, es, ed)
            fresh = qgtc.TiledAdjacency(n, adj.row_ptr, adj.kquad, tiles)
            busy = not ev.query()
            val_ptr, val_row, nnz = tiled._value_index(fresh)
            r, c = tiled.edge_endpoints(fresh)
            got = nnz, val_ptr.cpu(), val_row.cpu(), r.cpu(), c.cpu(), slots.cpu()
        torch.cuda.synchronize(env.dev)
        return busy, got

    with torch.cuda.device(env.dev):
        nnz, val_ptr, val_row, r, c, slots = until_sensitive(attempt)
    assert nnz == row.size and np.array_equal(val_ptr.numpy(), want_ptr) and np.array_equal(val_row.numpy(), want_row)
    assert np.array_equal(r.numpy(), row) and np.array_equal(c.numpy(), col)
    assert torch.equal(slots, torch.arange(row.size))


def _live(env, transposed):
    from qgtc_ppopp22_amd import tiled

    torch, n = env.torch, N_NODES
    src, dst, _, _, data = _case()
    adj = warm_adjacency(env, src, dst, n)
    a = adj.T if transposed else adj
    v, X, dY = bufs = [empty(env, t.shape, torch.float32) for t in data[0]]

    def run():
        Xg, vg = X.clone().requires_grad_(True), v.clone().requires_grad_(True)
        Y = env.Q.tiledAggregate(a, Xg, edge_weight=vg)
        gX, gv = torch.autograd.grad(Y, (Xg, vg), dY)
        return [Y.detach(), gX, gv, tiled.tiledSDDMM(a, dY, X)]

    def want(d):
        vals, Xn, dYn = d
        return [em.weighted_f32(src, dst, n, Xn, vals, transposed), em.weighted_f32(src, dst, n, dYn, vals, not transposed),
                em.sddmm_f32(src, dst, n, dYn, Xn, transposed), em.sddmm_f32(src, dst, n, dYn, Xn, transposed)]

    return Live(torch, bufs, data, [[np.asarray(w, dtype=np.float32) for w in want(d)] for d in data], run=run, keep=adj)


@pytest.mark.parametrize("transposed", [False, True])
def test_weighted_launch_and_sddmm_on_a_side_stream_and_under_capture(qgtc, oracle, transposed):
    import torch

    live = _live(env_of(qgtc, oracle, torch), transposed)
    what = f"weighted aggregate and SDDMM, {'adj.T' if transposed else 'adj'}"
    ordering_probe(torch, qgtc, live, what)
    capture_and_replay(torch, qgtc, live, what)
