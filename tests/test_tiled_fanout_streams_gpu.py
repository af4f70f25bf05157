"""Fixed-fanout sampling off the default stream, under graph capture and on recycled, poisoned memory (include/qgtc_fanout.h): the
selection launches and the sampled aggregates take the handle of torch's current stream, so behind a head start of plain torch work on a
side stream they see operands a producer wrote on that stream, and a captured graph replays selection, forward and backward on new
contents of the operands - one sample, because k and the seed are kernel arguments. On memory whose every word is a poison pattern
(tests/dirty_memory.py) ``thr`` and every output are written whole. All checks are bit for bit: the thresholds against
tests/tiled_fanout_model.py, the rest against the unmasked operators on the adjacency packed from the kept edges. The machine's
GPU_MAX_HW_QUEUES is left alone."""
import numpy as np
import pytest

import dirty_memory as dmem
import tiled_fanout_model as fm
from tiled_model import random_edges

pytestmark = pytest.mark.gpu

MODULE = "tests/test_tiled_fanout_streams_gpu.py"
N_COLS, K, SEED = 40, 3, 0x0123456789ABCDEF


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def setup():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    import QGTC

    n = 600
    rng = np.random.default_rng(41)
    src, dst = (np.asarray(a, dtype=np.int64) for a in random_edges(rng, n, 6 * n + 5))
    adj = QGTC.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    adj.T   # the column index, before any capture
    data = [tuple(rng.standard_normal(s).astype(np.float32) for s in ((n, N_COLS), (n, N_COLS), (n,), (n,))) for _ in range(3)]   # X, dY, p, q
    scales = tuple(_dev(torch, rng.uniform(0.5, 2.0, n).astype(np.float32)) for _ in range(2))
    kept = {axis: QGTC.pack_edges_tiled(*(_dev(torch, t) for t in fm.kept_edges(src, dst, n, K, SEED, axis)), n) for axis in fm.AXES}
    for k in kept.values():
        k.T
    thr = {axis: fm.thresholds(src, dst, n, K, SEED, axis) for axis in fm.AXES}
    return torch, QGTC, n, adj, data, scales, kept, thr


def _both_ways(torch, QGTC, a, X, dY, p, q, r, c, **kw):
    """forward and backward of the three modes of tiledAggregate on view `a`"""
    X, p, q = X.clone().requires_grad_(True), p.clone().requires_grad_(True), q.clone().requires_grad_(True)
    Ys = QGTC.tiledAggregate(a, X, r, c, **kw)
    Ym = QGTC.tiledAggregate(a, X, reduce="max", **kw)
    Ya = QGTC.tiledAggregate(a, X, attn=(p, q), **kw)
    grads = torch.autograd.grad(Ys, X, dY) + torch.autograd.grad(Ym, X, dY) + torch.autograd.grad(Ya, (X, p, q), dY)
    return [Ys.detach(), Ym.detach(), Ya.detach()] + list(grads)


def _run(torch, QGTC, a, bufs, scales):
    """the selection on both views, then everything with the pair (own form, one more selection each) and with the other view's sample
    (nbr form)"""
    from qgtc_ppopp22_amd import fanout

    own, other = fanout.sample_fanout(a, K, SEED), fanout.sample_fanout(a.T, K, SEED)
    return ([own.thr, other.thr] + _both_ways(torch, QGTC, a, *bufs, *scales, fanout=(K, SEED))
            + _both_ways(torch, QGTC, a, *bufs, *scales, fanout=other))


def _wants(torch, QGTC, transposed, d, scales, kept, thr):
    axis, other = ("col", "row") if transposed else ("row", "col")
    view = (lambda k: k.T) if transposed else (lambda k: k)
    bufs = tuple(_dev(torch, t) for t in d)
    return ([_dev(torch, thr[axis].view(np.int32)), _dev(torch, thr[other].view(np.int32))]
            + _both_ways(torch, QGTC, view(kept[axis]), *bufs, *scales) + _both_ways(torch, QGTC, view(kept[other]), *bufs, *scales))


def _same(torch, got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and torch.equal(g.view(torch.int32), w.view(torch.int32)), (what, i)


def _head_start(torch):
    a, b = torch.rand(2048, 2048, device="cuda"), torch.rand(2048, 2048, device="cuda")
    for _ in range(8):
        a = torch.mm(a, b).clamp_(0, 1)   # work queued ahead on the current (side) stream
    return a


@pytest.mark.parametrize("transposed", [False, True])
def test_selection_and_aggregates_on_a_side_stream_and_under_capture(setup, transposed):
    torch, QGTC, n, adj, data, scales, kept, thr = setup
    a = adj.T if transposed else adj
    wants = [_wants(torch, QGTC, transposed, d, scales, kept, thr) for d in data]
    pinned = [tuple(torch.from_numpy(t).pin_memory() for t in d) for d in data]
    bufs = tuple(torch.zeros_like(_dev(torch, t)) for t in data[0])
    for t, p in zip(bufs, pinned[0]):
        t.copy_(p)
    _same(torch, _run(torch, QGTC, a, bufs, scales), wants[0], "eager")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _head_start(torch)
        for t, p in zip(bufs, pinned[1]):
            t.copy_(p, non_blocking=True)   # the pending producer on this stream
        got = _run(torch, QGTC, a, bufs, scales)
    side.synchronize()
    _same(torch, got, wants[1], "side stream: a launch on another stream would have read the previous operands")
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = _run(torch, QGTC, a, bufs, scales)
    for k in (2, 0):
        for t, p in zip(bufs, pinned[k]):
            t.copy_(p)
        got[0].fill_(-1)                    # the replay writes thr again
        graph.replay()
        torch.cuda.synchronize()
        _same(torch, got, wants[k], f"replay {k}")


@pytest.mark.parametrize("transposed", [False, True])
def test_on_recycled_poisoned_memory(setup, transposed):
    """thr, every output, every statistic kept for the backward and every gradient come from torch.empty: under both poison patterns they
    equal the results on the re-packed adjacency, and each other."""
    torch, QGTC, n, adj, data, scales, kept, thr = setup
    a = adj.T if transposed else adj
    dev = torch.device("cuda", torch.cuda.current_device())
    want = [t.cpu() for t in _wants(torch, QGTC, transposed, data[0], scales, kept, thr)]
    bufs = tuple(_dev(torch, t) for t in data[0])
    _run(torch, QGTC, a, bufs, scales)      # warm-up outside the poisoned region: handles and workspaces exist
    results = []
    for pattern in dmem.PATTERNS:
        with dmem.dirty(torch, dev, pattern, inputs=list(bufs) + list(scales)) as d:
            dmem.announce(MODULE, d)
            got = [t.detach().cpu() for t in _run(torch, QGTC, a, bufs, scales)]
        dmem.same_bits(got, want, f"fanout on memory poisoned with {pattern:#010x}")
        results.append(got)
    dmem.same_bits(results[0], results[1], "one pattern against the other")
