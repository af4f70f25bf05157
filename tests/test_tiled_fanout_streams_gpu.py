"""Fixed-fanout sampling off the default stream, under graph capture and on recycled, poisoned memory (include/qgtc_fanout.h): the
selection launches and the sampled aggregates take the handle of torch's current stream. One ``Live`` case of tests/stream_cases.py per
view: ``ordering_probe`` puts selection, forward and backward behind a timed head start on three fresh side streams, where they must see
operands a producer wrote on that stream, and ``capture_and_replay`` replays them on three new contents of the operands - one sample,
because k and the seed are kernel arguments, so both ``thr`` are filled with -1 before every replay. On memory whose every word is a
poison pattern (tests/dirty_memory.py) ``thr`` and every output are written whole. All checks are bit for bit: the thresholds against
tests/tiled_fanout_model.py, the rest against the unmasked operators on the adjacency packed from the kept edges. The machine's
GPU_MAX_HW_QUEUES is left alone."""
import numpy as np
import pytest

import dirty_memory as dmem
import tiled_fanout_model as fm
from stream_cases import Live, capture_and_replay, empty, env_of, ordering_probe, warm_adjacency
from tiled_model import random_edges

pytestmark = pytest.mark.gpu

MODULE = "tests/test_tiled_fanout_streams_gpu.py"
N_COLS, K, SEED = 40, 3, 0x0123456789ABCDEF


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def setup(qgtc, oracle):
    import torch

    env = env_of(qgtc, oracle, torch)
    n = 600
    rng = np.random.default_rng(41)
    src, dst = (np.asarray(a, dtype=np.int64) for a in random_edges(rng, n, 6 * n + 5))
    adj = warm_adjacency(env, src, dst, n)
    data = [tuple(rng.standard_normal(s).astype(np.float32) for s in ((n, N_COLS), (n, N_COLS), (n,), (n,))) for _ in range(3)]   # X, dY, p, q
    scales = tuple(_dev(torch, rng.uniform(0.5, 2.0, n).astype(np.float32)) for _ in range(2))
    data.append(tuple(rng.standard_normal(s).astype(np.float32) for s in ((n, N_COLS), (n, N_COLS), (n,), (n,))))   # the fourth content
    kept = {axis: qgtc.pack_edges_tiled(*(_dev(torch, t) for t in fm.kept_edges(src, dst, n, K, SEED, axis)), n) for axis in fm.AXES}
    for k in kept.values():
        k.T
    thr = {axis: fm.thresholds(src, dst, n, K, SEED, axis) for axis in fm.AXES}
    return env, adj, data, scales, kept, thr


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
    """the model's thresholds and the unmasked operators on the adjacencies packed from the kept edges, as CPU tensors"""
    axis, other = ("col", "row") if transposed else ("row", "col")
    view = (lambda k: k.T) if transposed else (lambda k: k)
    bufs = tuple(_dev(torch, t) for t in d)
    want = ([_dev(torch, thr[axis].view(np.int32)), _dev(torch, thr[other].view(np.int32))]
            + _both_ways(torch, QGTC, view(kept[axis]), *bufs, *scales) + _both_ways(torch, QGTC, view(kept[other]), *bufs, *scales))
    return [t.cpu() for t in want]


def _live(env, transposed, adj, data, scales, kept, thr):
    torch = env.torch
    a = adj.T if transposed else adj
    wants = [_wants(torch, env.Q, transposed, d, scales, kept, thr) for d in data]   # on the default stream, before any probe
    bufs = [empty(env, t.shape, torch.float32) for t in data[0]]
    return Live(torch, bufs, data, wants, run=lambda: _run(torch, env.Q, a, bufs, scales), keep=adj, refill=(0, 1))


@pytest.mark.parametrize("transposed", [False, True])
def test_selection_and_aggregates_on_a_side_stream_and_under_capture(setup, transposed):
    env = setup[0]
    live = _live(env, transposed, *setup[1:])
    what = f"fanout selection and sampled aggregates, {'adj.T' if transposed else 'adj'}"
    ordering_probe(env.torch, env.Q, live, what)
    capture_and_replay(env.torch, env.Q, live, what)


@pytest.mark.parametrize("transposed", [False, True])
def test_on_recycled_poisoned_memory(setup, transposed):
    """thr, every output, every statistic kept for the backward and every gradient come from torch.empty: under both poison patterns they
    equal the results on the re-packed adjacency, and each other."""
    env, adj, data, scales, kept, thr = setup
    torch, QGTC = env.torch, env.Q
    a = adj.T if transposed else adj
    dev = torch.device("cuda", torch.cuda.current_device())
    want = _wants(torch, QGTC, transposed, data[0], scales, kept, thr)
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
