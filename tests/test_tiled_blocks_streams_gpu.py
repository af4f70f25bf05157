"""Mini-batch sampling off the default stream, under graph capture and on recycled, poisoned memory (include/qgtc_blocks.h): the masked
selection, the frontier, one sampled aggregate under the masked sample and ``sample_blocks`` take the handle of torch's current stream.
One ``Live`` case of tests/stream_cases.py per view: ``ordering_probe`` puts them behind a timed head start on three fresh side streams,
where they must see the masks and features a producer wrote on that stream, and ``capture_and_replay`` replays them on three new
contents - the masks and thr are read on the device, so a replay follows them; thr, counts and the frontier words are filled with -1
before every replay. On memory whose every word is a poison pattern (tests/dirty_memory.py) thr, counts, every frontier word and every
output are written whole: the frontier has no clear to lean on. All checks are bit for bit: thresholds, counts, frontiers and blocks
against tests/tiled_blocks_model.py, the aggregate against the plain operator on the adjacency packed from the kept edges. The machine's
GPU_MAX_HW_QUEUES is left alone."""
import numpy as np
import pytest

import dirty_memory as dmem
import tiled_blocks_model as bm
from stream_cases import Live, capture_and_replay, empty, env_of, ordering_probe, same, warm_adjacency
from tiled_model import random_edges

pytestmark = pytest.mark.gpu

MODULE = "tests/test_tiled_blocks_streams_gpu.py"
N_COLS, K, FANOUTS, SEED = 40, 3, (3, 2), 0x0123456789ABCDEF


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def setup(qgtc, oracle):
    import torch

    env = env_of(qgtc, oracle, torch)
    n = 600
    rng = np.random.default_rng(43)
    src, dst = (np.asarray(a, dtype=np.int64) for a in random_edges(rng, n, 6 * n + 5))
    adj = warm_adjacency(env, src, dst, n)
    data = []   # four inputs that differ in everything a replay reads: X, dY, the rows, the neighbours, the batch's seeds
    for i in range(4):
        seeds = np.zeros(n, dtype=bool)
        seeds[rng.permutation(n)[:15 + 5 * i]] = True
        data.append((rng.standard_normal((n, N_COLS)).astype(np.float32), rng.standard_normal((n, N_COLS)).astype(np.float32),
                     bm.bitmap(np.arange(n) % 3 == i % 3), bm.bitmap(rng.random(n) < 0.5), bm.bitmap(seeds)))
    return env, n, src, dst, adj, data


def _run(torch, QGTC, a, bufs):
    from qgtc_ppopp22_amd import fanout

    X, dY, row, nbr, seeds = bufs
    s = fanout.sample_fanout(a, K, SEED, row_mask=row, nbr_mask=nbr)
    Xg = X.clone().requires_grad_(True)
    Y = QGTC.tiledAggregate(a, Xg, s.mean_scale(), fanout=s)
    dX, = torch.autograd.grad(Y, Xg, dY)
    out = [s.thr, s.counts, fanout.frontier(s), fanout.frontier(s, include=True), Y.detach(), dX]
    for b in fanout.sample_blocks(a, seeds, FANOUTS, SEED):
        out += [b.sample.thr, b.sample.counts, b.inputs]
    return out


def _wants(torch, QGTC, transposed, n, src, dst, d):
    """the model's thresholds, counts, frontiers and blocks, and the plain operator on the adjacency packed from the kept edges, as CPU
    tensors"""
    axis = "col" if transposed else "row"
    X, dY, row, nbr, seeds = d
    row, nbr, seeds = (bm.flags_of(t, n) for t in (row, nbr, seeds))
    thr, kept = bm.thresholds_counts(src, dst, n, K, SEED, axis, row, nbr)
    kadj = QGTC.pack_edges_tiled(*(_dev(torch, t) for t in bm.kept_edges(src, dst, n, K, SEED, axis, row, nbr)), n)
    ka = kadj.T if transposed else kadj
    Xg = _dev(torch, X).requires_grad_(True)
    Y = QGTC.tiledAggregate(ka, Xg, ka.mean_scale())
    dX, = torch.autograd.grad(Y, Xg, _dev(torch, dY))
    out = [_dev(torch, thr.view(np.int32)), _dev(torch, kept), _dev(torch, bm.bitmap(bm.frontier(src, dst, n, K, SEED, axis, row, nbr))),
           _dev(torch, bm.bitmap(bm.frontier(src, dst, n, K, SEED, axis, row, nbr, row))), Y.detach(), dX]
    for b in bm.blocks(src, dst, n, axis, seeds, FANOUTS, SEED):
        out += [_dev(torch, b["thr"].view(np.int32)), _dev(torch, b["kept"]), _dev(torch, bm.bitmap(b["inputs"]))]
    return [t.cpu() for t in out]


def _live(env, transposed, n, src, dst, adj, data):
    torch = env.torch
    a = adj.T if transposed else adj
    wants = [_wants(torch, env.Q, transposed, n, src, dst, d) for d in data]   # on the default stream, before any probe
    bufs = [empty(env, t.shape, torch.from_numpy(t).dtype) for t in data[0]]
    return Live(torch, bufs, data, wants, run=lambda: _run(torch, env.Q, a, bufs), keep=adj, refill=(0, 1, 2, 3))


@pytest.mark.parametrize("transposed", [False, True])
def test_on_a_side_stream_and_under_capture(setup, transposed):
    env = setup[0]
    live = _live(env, transposed, *setup[1:])
    what = f"mini-batch sampling, {'adj.T' if transposed else 'adj'}"
    ordering_probe(env.torch, env.Q, live, what)
    capture_and_replay(env.torch, env.Q, live, what)
    assert not same(live.expected[1][2], live.expected[2][2]), "the frontiers of contents 1 and 2 differ"


@pytest.mark.parametrize("transposed", [False, True])
def test_on_recycled_poisoned_memory(setup, transposed):
    """thr, counts, the frontiers, the blocks' bitmaps, the aggregate and its gradient come from torch.empty: under both poison patterns
    they equal the model and the re-packed adjacency, and each other. A frontier kernel that skipped a word would leave the pattern."""
    env, n, src, dst, adj, data = setup
    torch, QGTC = env.torch, env.Q
    a = adj.T if transposed else adj
    dev = torch.device("cuda", torch.cuda.current_device())
    want = _wants(torch, QGTC, transposed, n, src, dst, data[0])
    bufs = tuple(_dev(torch, t) for t in data[0])
    _run(torch, QGTC, a, bufs)              # warm-up outside the poisoned region: handles and workspaces exist
    results = []
    for pattern in dmem.PATTERNS:
        with dmem.dirty(torch, dev, pattern, inputs=list(bufs)) as d:
            dmem.announce(MODULE, d)
            got = [t.detach().cpu() for t in _run(torch, QGTC, a, bufs)]
        dmem.same_bits(got, want, f"mini-batch sampling on memory poisoned with {pattern:#010x}")
        results.append(got)
    dmem.same_bits(results[0], results[1], "one pattern against the other")
