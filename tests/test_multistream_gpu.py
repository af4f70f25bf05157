"""The entries that fork onto the binding's pool streams (class FORKS of tests/stream_contract.py): QGTC.bitMM2Bit_enqueue_streams,
BatchedGemm.run_per_problem and the driver's BatchedEpoch.run_per_batch on top of it. Eager only: a multi-stream launch is never captured.

Every test is the ordering probe of tests/stream_cases.py in the multi-stream form: content 0 in the operands, synchronise; then on the
CALLING stream (the default one, or a side stream) the head start, the copy of content 1, a NaN prefill of the outputs, the call, and a
consumer queued right behind it on the calling stream. The fork makes the pool streams wait for the copy and the prefill; the join makes
the consumer wait for the pool streams. Bit for bit against the oracle."""
import contextlib

import numpy as np
import pytest

import stream_cases as sc
from helpers import oracle_chain  # noqa: F401  (the chains' oracle: through stream_cases._grouped_live)
from qgtc_ppopp22_amd.shapes import cols_shape, rows_shape

pytestmark = pytest.mark.gpu

SHAPES = [(129, 513, 100, 3, 2, 5), (1213, 1213, 128, 1, 2, 2)]


@pytest.fixture(scope="module")
def env(qgtc, oracle):
    import torch

    return sc.env_of(qgtc, oracle, torch)


@pytest.fixture(scope="module")
def mm_data(env):
    """Per shape: two contents (X, W words) and the oracle's rows-layout result of each."""
    data = {}
    for dims in SHAPES:
        M, K, N, a, w, ob = dims
        ops = [sc._mm_operands(env.O, M, K, N, a, w, 4000 + k) for k in range(2)]
        data[dims] = (ops, [env.O.bitmm2bit(X, Wt, M, K, N, a, w, ob) for X, Wt in ops])
        assert not sc.same(data[dims][1][0], data[dims][1][1])
    return data


def _calling_stream(torch, side):
    return torch.cuda.stream(torch.cuda.Stream()) if side else contextlib.nullcontext()


def _pinned(torch, words, like):
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).reshape(like.shape).pin_memory()


def _reps(n):
    return sorted({r for r in (1, n - 1, n, n + 1, 50) if r >= 1})


@pytest.mark.parametrize("side", [False, True], ids=["default-stream", "side-stream"])
@pytest.mark.parametrize("dims", SHAPES, ids=lambda d: "x".join(map(str, d[:3])))
@pytest.mark.parametrize("n,reps", [(n, r) for n in (1, 2, 3, 4, 8) for r in _reps(n)])
def test_enqueue_streams(env, mm_data, n, reps, dims, side):
    torch, Q = env.torch, env.Q
    M, K, N, a, w, ob = dims
    ops, want = mm_data[dims]
    bX, bW = torch.empty(rows_shape(M, K, a), dtype=torch.int32, device=env.dev), torch.empty(cols_shape(K, N, w), dtype=torch.int32, device=env.dev)
    staged = [(_pinned(torch, X, bX), _pinned(torch, Wt, bW)) for X, Wt in ops]
    outs = [torch.empty(rows_shape(M, N, ob), dtype=torch.int32, device=env.dev) for _ in range(n)]

    def attempt(scale):
        bX.copy_(staged[0][0])
        bW.copy_(staged[0][1])
        Q.bitMM2Bit_enqueue_streams(outs, bX, bW, M, K, N, a, w, ob, reps)          # (the pool streams exist, the kernel is loaded)
        torch.cuda.synchronize()
        with _calling_stream(torch, side):
            ev = sc.head_start(torch, env.dev, scale)
            bX.copy_(staged[1][0], non_blocking=True)
            bW.copy_(staged[1][1], non_blocking=True)
            for o in outs:
                o.fill_(sc.NAN_WORD)
            Q.bitMM2Bit_enqueue_streams(outs, bX, bW, M, K, N, a, w, ob, reps)
            busy = not ev.query()
            got = torch.stack(outs).cpu()            # a consumer on the calling stream, right behind the call: the join
        torch.cuda.synchronize()
        return busy, got
    reached = min(reps, n)
    untouched = np.full(want[1].size, sc.NAN_WORD, np.uint32)
    sc.probe_rounds(attempt, lambda got, which: sc.check(
        [got[i] for i in range(n)], [want[1]] * reached + [untouched] * (n - reached), f"n={n} reps={reps}, {which}",
        old=[want[0]] * reached + [untouched] * (n - reached), old_means="ran ahead of the calling stream (the fork is missing)"))


def test_enqueue_streams_rejects_mixed_outputs(env, mm_data):
    torch, Q = env.torch, env.Q
    M, K, N, a, w, ob = SHAPES[0]
    (X, Wt), _ = mm_data[SHAPES[0]][0][0], None
    bX = torch.from_numpy(X.view(np.int32)).reshape(rows_shape(M, K, a)).to(env.dev)
    bW = torch.from_numpy(Wt.view(np.int32)).reshape(cols_shape(K, N, w)).to(env.dev)
    good = torch.full(rows_shape(M, N, ob), sc.CANARY, dtype=torch.int32, device=env.dev)
    with pytest.raises(RuntimeError, match="int32"):
        Q.bitMM2Bit_enqueue_streams([good, good.clone().view(torch.float32)], bX, bW, M, K, N, a, w, ob, 2)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        Q.bitMM2Bit_enqueue_streams([good, torch.zeros(rows_shape(M, N, ob), dtype=torch.int32)], bX, bW, M, K, N, a, w, ob, 2)
    with pytest.raises(RuntimeError):
        Q.bitMM2Bit_enqueue_streams([], bX, bW, M, K, N, a, w, ob, 2)
    with pytest.raises(RuntimeError):
        Q.bitMM2Bit_enqueue_streams([good], bX, bW, M, K, N, a, w, ob, 0)
    if torch.cuda.device_count() > 1:
        with pytest.raises(RuntimeError, match="device"):
            Q.bitMM2Bit_enqueue_streams([good, good.to("cuda:1")], bX, bW, M, K, N, a, w, ob, 2)
    torch.cuda.synchronize()
    assert bool((good.cpu() == sc.CANARY).all()), "a rejected call launched"


# ---- BatchedGemm.run_per_problem ---------------------------------------------------------------------------------------------------------
DIMS = [(1213, 1213, 128), (1100, 1100, 128), (37, 37, 128), (640, 640, 128)]      # tests/test_gpu_parity.py::test_batched_matches_single
A_BITS, W_BITS, OB = 1, 2, 2


@pytest.fixture(scope="module")
def ragged(env):
    """Two contents of the ragged problems and the oracle's result of each in the three output modes."""
    from helpers import rand_q

    contents, want = [], []
    for k in range(2):
        rng = np.random.default_rng(21 + k)
        ops = []
        for (M, K, N) in DIMS:
            ops.append((env.O.pack(rand_q(rng, M, K, A_BITS, 0.01), A_BITS, False), env.O.pack(rand_q(rng, K, N, W_BITS), W_BITS, True)))
        contents.append(ops)
        want.append({0: [env.O.bitmm2bit(X, Wt, M, K, N, A_BITS, W_BITS, OB) for (X, Wt), (M, K, N) in zip(ops, DIMS)],
                     1: [env.O.bitmm2bit(X, Wt, M, K, N, A_BITS, W_BITS, OB, col=True) for (X, Wt), (M, K, N) in zip(ops, DIMS)],
                     2: [env.O.bitmm2int(X, Wt, M, K, N, A_BITS, W_BITS, True) for (X, Wt), (M, K, N) in zip(ops, DIMS)]})
    return contents, want


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("n_streams", [1, 2, 3, 4, 7, 32])
def test_run_per_problem(env, ragged, n_streams, mode):
    torch, Q = env.torch, env.Q
    contents, want = ragged
    Xs = [torch.empty(rows_shape(M, K, A_BITS), dtype=torch.int32, device=env.dev) for (M, K, N) in DIMS]
    Ws = [torch.empty(cols_shape(K, N, W_BITS), dtype=torch.int32, device=env.dev) for (M, K, N) in DIMS]
    staged = [[(_pinned(torch, X, bx), _pinned(torch, Wt, bw)) for (X, Wt), bx, bw in zip(ops, Xs, Ws)] for ops in contents]
    for (hx, hw), bx, bw in zip(staged[0], Xs, Ws):
        bx.copy_(hx)
        bw.copy_(hw)
    bg = Q.BatchedGemm(Xs, Ws, DIMS, A_BITS, W_BITS, OB, mode, True)

    def attempt(scale):
        for (hx, hw), bx, bw in zip(staged[0], Xs, Ws):
            bx.copy_(hx)
            bw.copy_(hw)
        bg.run_per_problem(n_streams)
        torch.cuda.synchronize()
        with torch.cuda.stream(torch.cuda.Stream()):
            ev = sc.head_start(torch, env.dev, scale)
            for (hx, hw), bx, bw in zip(staged[1], Xs, Ws):
                bx.copy_(hx, non_blocking=True)
                bw.copy_(hw, non_blocking=True)
            for o in bg.outs:
                o.view(torch.int32).fill_(sc.NAN_WORD)
            bg.run_per_problem(n_streams)
            busy = not ev.query()
            got = [o.cpu() for o in bg.outs]         # consumers on the calling stream: the join
        torch.cuda.synchronize()
        return busy, got
    sc.probe_rounds(attempt, lambda got, which: sc.check(got, want[1][mode], f"run_per_problem({n_streams}), mode {mode}, {which}", old=want[0][mode],
                                                        old_means="ran ahead of the calling stream (the fork is missing)"))
    bg.run()                                      # and the grouped launch of the same plan agrees
    sc.check([o.cpu() for o in bg.outs], want[1][mode], f"run(), mode {mode}")


def test_run_per_problem_rejects_stream_counts_out_of_range(env):
    torch, Q = env.torch, env.Q
    X = torch.zeros(rows_shape(8, 128, 1), dtype=torch.int32, device=env.dev)
    W = torch.zeros(cols_shape(128, 8, 1), dtype=torch.int32, device=env.dev)
    bg = Q.BatchedGemm([X], [W], [(8, 128, 8)], 1, 1, 1, 0, True)
    bg.outs[0].fill_(sc.CANARY)
    for bad in (0, 33, -1):
        with pytest.raises(RuntimeError, match="n_streams"):
            bg.run_per_problem(bad)
    torch.cuda.synchronize()
    assert bool((bg.outs[0].cpu() == sc.CANARY).all())


# ---- chained stages over the streams ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_streams", [1, 3, 4])
@pytest.mark.parametrize("chain,gin,bits", [("reference", False, 2), ("correct", False, 2), ("correct", True, 4), ("reference", True, 4)])
def test_run_per_batch_chains_its_stages(env, chain, gin, bits, n_streams):
    """The six stages consume each other's outputs: batch i stays on stream i % n, and every stage forks from and joins the calling
    stream, so a missing fork or join between two stages shows as a wrong final output."""
    torch = env.torch
    live = sc._grouped_live(env, chain, gin, planned=False, b=bits, seed=20 + n_streams)
    plan = live.plan

    def attempt(scale):
        live.load(0)
        plan.run_per_batch(n_streams)
        torch.cuda.synchronize()
        with torch.cuda.stream(torch.cuda.Stream()):
            ev = sc.head_start(torch, env.dev, scale)
            live.load(1)
            for g in plan.stages:
                for o in g.outs:
                    o.view(torch.int32).fill_(sc.NAN_WORD)
            outs = plan.run_per_batch(n_streams)
            busy = not ev.query()
            got = [o.cpu() for o in outs]
        torch.cuda.synchronize()
        return busy, got
    sc.probe_rounds(attempt, lambda got, which: sc.check(got, live.expected[1], f"run_per_batch({n_streams}) {chain} gin={gin}, {which}",
                                                        old=live.expected[0], old_means="ran ahead of the calling stream"))
    sc.check([o.cpu() for o in plan.run()], live.expected[1], "run() of the same plan")
