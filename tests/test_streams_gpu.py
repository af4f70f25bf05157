"""Every asynchronous entry of the stream contract (tests/stream_contract.py) off the default stream and under graph capture.

test_ordering_on_a_side_stream: the eager probe of tests/stream_cases.py::ordering_probe. The head start is plain torch.mm work timed
with HIP events once per process and repeated until it takes at least 5 ms. Measured on an MI355X: 5 x torch.mm(4096^2 float32) = 5.07
to 5.21 ms in six runs, 8 x = 7.91 ms in one. The host needs microseconds to queue the copy and the operator behind it,
and every probe checks that the head start was still running when it had (an event behind it is still pending), so an operator on any
other stream reads the buffers' previous content. The figure sets the probe's sensitivity, it is no threshold on the code under test.
Each probe runs on three consecutive side streams (stream_cases.probe_rounds: streams share four hardware queues).

test_capture_and_replay: one warm-up call on a side stream, one captured call, three replays on new contents.

test_lazy_caches_move_to_a_second_stream: the rule INTEGRATION.md states for TiledAdjacency's caches.

Bit for bit against the CPU oracle and the NumPy models everywhere."""
import numpy as np
import pytest

import stream_cases as sc
from stream_contract import ASYNC, names_of

pytestmark = pytest.mark.gpu


def _params(kind):
    """Every case of tests/stream_cases.py once, and a failing placeholder for an ASYNC entry of the contract that has none."""
    out = [pytest.param(c, id=c.id) for c in sc.CASES if getattr(c, kind) and not c.raw]
    out += [pytest.param(name, id=f"NO-CASE-{name}") for name in names_of(ASYNC)
            if not any(getattr(c, kind) and not c.raw for c in sc.cases_of(name))]
    return out


@pytest.fixture(scope="module")
def env(qgtc, oracle):
    import torch

    return sc.env_of(qgtc, oracle, torch)


@pytest.mark.parametrize("case", _params("probe"))
def test_ordering_on_a_side_stream(env, case):
    assert not isinstance(case, str), f"{case} is asynchronous by the contract and has no ordering probe"
    sc.ordering_probe(env.torch, env.Q, case.build(env), f"{'/'.join(case.entries)} [{case.id}]")


@pytest.mark.parametrize("case", _params("capture"))
def test_capture_and_replay(env, case):
    assert not isinstance(case, str), f"{case} is asynchronous by the contract and has no capture case"
    sc.capture_and_replay(env.torch, env.Q, case.build(env), f"{'/'.join(case.entries)} [{case.id}]")


def test_the_head_start_is_long_enough(env):
    fill = sc.filler_for(env.torch, env.dev)
    assert fill.ms >= sc.FILLER_MIN_MS
    print(f"head start: {fill.reps} x torch.mm = {fill.ms:.2f} ms")


@pytest.mark.parametrize("turn", range(sc.PROBE_ROUNDS))        # consecutive pool streams: stream_cases.probe_rounds says why
def test_lazy_caches_move_to_a_second_stream(env, turn):
    """A fresh adjacency whose caches are first touched on stream s (behind the head start and the copy of the adjacency's content), used
    right behind them on s; then, after s2.wait_stream(s), the same cached tensors on a second stream s2. Both equal the model."""
    torch, Q = env.torch, env.Q
    gs = sc.cache_graphs()
    bufs = sc._adjacency_buffers(env, gs)
    X = torch.from_numpy(np.random.default_rng(3).normal(size=(sc.CACHE_N, 24)).astype(np.float32)).to(env.dev)
    want_old, want = (sc.cache_expected(g[0], g[1], X.cpu().numpy()) for g in (gs[0], gs[1]))
    pinned = [[torch.from_numpy(np.ascontiguousarray(a).view(np.int32) if a.dtype == np.uint32 else np.ascontiguousarray(a)).reshape(b.shape).pin_memory()
               for a, b in zip(g[2], bufs)] for g in gs[:2]]
    for b, h in zip(bufs, pinned[0]):
        b.copy_(h)
    torch.cuda.synchronize()
    adj = Q.TiledAdjacency(sc.CACHE_N, *bufs)
    sc.cache_run(Q, Q.TiledAdjacency(sc.CACHE_N, *bufs), X)          # another adjacency object: the kernels are loaded, `adj` stays fresh
    torch.cuda.synchronize()
    assert adj._other is None and adj._degrees is None and adj._sym is None
    s, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s):
        ev = sc.head_start(torch, env.dev, 2)
        for b, h in zip(bufs, pinned[1]):
            b.copy_(h, non_blocking=True)
        outs = sc.cache_run(Q, adj, X)
        assert not ev.query(), "the head start ended before the caches were queued: the probe could not see a mis-streamed launch"
        first = [o.cpu() for o in outs]
    sc.check(first, want, "caches built and used on s", old=want_old)
    cached = (adj.T, adj.mean_scale(), adj.sym_scale())
    s2.wait_stream(s)
    with torch.cuda.stream(s2):
        sc.head_start(torch, env.dev)
        second = [o.cpu() for o in sc.cache_run(Q, adj, X)]
    assert adj.T is cached[0] and adj.mean_scale() is cached[1] and adj.sym_scale() is cached[2]      # used, not rebuilt
    sc.check(second, want, "the same caches on s2 after s2.wait_stream(s)")
    torch.cuda.synchronize()


@pytest.mark.parametrize("turn", range(sc.PROBE_ROUNDS))
def test_backward_builds_the_transposed_view_on_the_stream_it_runs_on(env, turn):
    """tiledAggregate's backward is the first to ask for adj.T (tiled.py: _TiledAggregate.backward): under a side stream the column
    index is built there, behind the forward, and the gradient equals the model."""
    from tiled_sym_model import aggregate_f32_src

    torch, Q = env.torch, env.Q
    n, N = 600, 24
    src, dst = sc.graph(n, 31)
    adj = Q.pack_edges_tiled(torch.from_numpy(src).to(env.dev), torch.from_numpy(dst).to(env.dev), n)
    assert adj._other is None
    rng = np.random.default_rng(32)
    Xs = [rng.normal(size=(n, N)).astype(np.float32) for _ in range(2)]
    G = rng.normal(size=(n, N)).astype(np.float32)
    X = torch.from_numpy(Xs[0]).to(env.dev).requires_grad_(True)
    dG = torch.from_numpy(G).to(env.dev)
    staged = torch.from_numpy(Xs[1]).pin_memory()
    warm = Q.pack_edges_tiled(torch.from_numpy(src).to(env.dev), torch.from_numpy(dst).to(env.dev), n)      # loads the kernels; `adj` stays fresh
    torch.autograd.grad(Q.tiledAggregate(warm, X), X, dG)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ev = sc.head_start(torch, env.dev, 2)
        with torch.no_grad():
            X.copy_(staged, non_blocking=True)
        y = Q.tiledAggregate(adj, X)
        (gx,) = torch.autograd.grad(y, X, dG)
        assert not ev.query(), "the head start ended before the backward was queued: the probe could not see a mis-streamed launch"
        got = [y.detach().cpu(), gx.cpu()]
    assert adj._other is not None
    sc.check(got, [aggregate_f32_src(src, dst, n, Xs[1], False), aggregate_f32_src(src, dst, n, G, True)], "tiledAggregate under a side stream",
             old=[aggregate_f32_src(src, dst, n, Xs[0], False), aggregate_f32_src(src, dst, n, G, True)])
    torch.cuda.synchronize()


@pytest.mark.parametrize("dims", sc.ENQUEUE_SMALL[:1] + sc.ENQUEUE_BIG[:1])
def test_enqueue_rejects_a_bad_output_and_launches_nothing(env, dims):
    """An `out` one word short, of another dtype, or on the CPU raises; the buffers stay as they were (canaries everywhere)."""
    torch, Q = env.torch, env.Q
    for cols in (False, True):
        live = sc.enqueue_live(env, *dims, 3, cols)
        M, K, N, a, w, ob, reps, _ = live.args
        live.load(1)
        need = live.out.numel()
        short = torch.full((need - 1 + 64,), sc.CANARY, dtype=torch.int32, device=env.dev)
        with pytest.raises(RuntimeError):
            Q.bitMM2Bit_enqueue(short[: need - 1], live.bufs[0], live.bufs[1], M, K, N, a, w, ob, reps, cols)
        with pytest.raises(RuntimeError, match="int32"):
            Q.bitMM2Bit_enqueue(short[: need - 1].view(torch.float32), live.bufs[0], live.bufs[1], M, K, N, a, w, ob, reps, cols)
        wrong = torch.full((need + 64,), 1.5, dtype=torch.float32, device=env.dev)
        with pytest.raises(RuntimeError, match="int32"):
            Q.bitMM2Bit_enqueue(wrong[:need], live.bufs[0], live.bufs[1], M, K, N, a, w, ob, reps, cols)
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            Q.bitMM2Bit_enqueue(torch.zeros(need, dtype=torch.int32), live.bufs[0], live.bufs[1], M, K, N, a, w, ob, reps, cols)
        with pytest.raises(RuntimeError):
            Q.bitMM2Bit_enqueue(live.out, live.bufs[0], live.bufs[1], M, K, N, a, w, ob, 0, cols)
        torch.cuda.synchronize()
        assert bool((short.cpu() == sc.CANARY).all()) and bool((wrong.cpu() == 1.5).all()), "a rejected call wrote into its output"
        # and the accepted call on the same operands gives bitMM2Bit / bitMM2Bit_col
        Q.bitMM2Bit_enqueue(live.out, live.bufs[0], live.bufs[1], M, K, N, a, w, ob, reps, cols)
        ref = (Q.bitMM2Bit_col if cols else Q.bitMM2Bit)(live.bufs[0], live.bufs[1], M, K, N, a, w, ob)
        assert torch.equal(live.out, ref.reshape(-1))
        sc.check([live.out.cpu()], [live.expected[1][0]], f"enqueue cols={cols}")
