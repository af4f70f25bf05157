"""Whole modules under graph capture (qgtc_ppopp22_amd/conv.py): the quantised GCNConv_Qnt on a dense adjacency and on a TiledAdjacency
(sum, mean, float_out), and one training step of the float GCNConv(norm="sym") - forward, loss, backward and the SGD step in one graph.
Warm-up on a side stream (it packs the weights and builds the adjacency's lazy caches), one capture, three replays on new inputs; every
replay equals the NumPy model of that input and the bits of the eager module. Only linear graphs: nothing here forks a stream."""
import numpy as np
import pytest

import stream_cases as sc

pytestmark = pytest.mark.gpu

N_NODES, F, H, C, WB, AB = 600, 40, 24, 7, 2, 3


def _low(q, b):
    return np.asarray(q).astype(np.int64) & ((1 << b) - 1)          # only bits 0 .. b-1 are packed


def qnt_model(oracle, src, dst, n, X, Wi, Wo, aggr, float_out):
    """GCNConv_Qnt on the quantised adjacency of an edge list, in integers (and the float32 epilogues of the scaled / float products)."""
    from oracle.qgtc_oracle import np_quantize, np_requant
    from tiled_float_model import aggregate_f32
    from tiled_model import aggregate
    from tiled_scaled_model import degrees, mean_scale, scaled

    rq = lambda c: _low(np_requant(np.asarray(c).astype(np.int32), AB), AB)   # noqa: E731
    qX, qWi, qWo = _low(np_quantize(X, AB), AB), _low(np_quantize(Wi, WB), WB), _low(np_quantize(Wo, WB), WB)
    scale = mean_scale(degrees(src, dst, n)[0]) if aggr == "mean" else None
    c1 = aggregate(src, dst, n, rq(qX @ qWi))
    h = _low(oracle.quantize(scaled(c1, scale), AB), AB) if aggr == "mean" else rq(c1)
    if float_out:
        # the module calls bitMM2Int with its default pad_128=False on weights packed with PAD128 lines: the oracle reads them the same way
        # (tests/test_tiled_float_gpu.py::_model_forward)
        hw = oracle.bitmm2int(oracle.pack(h, AB), oracle.val2bit(Wo, WB, True), n, Wo.shape[0], Wo.shape[1], AB, WB)
        return aggregate_f32(src, dst, n, hw, False, scale)
    c2 = aggregate(src, dst, n, rq(h @ qWo))
    return scaled(c2, scale) if aggr == "mean" else c2.astype(np.float32)


def _sparse(rng, shape, top):
    """Mostly values that quantise to 0 and one in twelve spread over the quantiser's range (edge values included): with dense inputs
    every product of the module runs into requant's clamp and the output no longer depends on X."""
    x = rng.uniform(0.0, 0.45, size=shape)                 # (a negative value quantises to 1, kernel.h:39-44)
    x = np.where(rng.random(shape) < 1.0 / 12, rng.uniform(0.4, top + 1.0, size=shape), x).astype(np.float32)
    x.flat[:7] = [np.nan, -0.0, 0.5, 1.5, 2.5, top, -1.0][: min(7, x.size)]
    return x


@pytest.fixture(scope="module")
def env(qgtc, oracle):
    import torch

    return sc.env_of(qgtc, oracle, torch)


@pytest.mark.parametrize("adjacency,aggr,float_out", [("dense", "sum", False), ("tiled", "sum", False), ("tiled", "mean", False),
                                                      ("tiled", "sum", True), ("tiled", "mean", True)])
def test_gcnconv_qnt_under_capture(env, adjacency, aggr, float_out):
    from qgtc_ppopp22_amd.conv import GCNConv_Qnt
    from tiled_model import set_cells

    torch, n = env.torch, N_NODES
    src, dst = sc.graph(n, 41)
    cells = set_cells(src, dst, n)
    s1, d1 = cells // n, cells % n            # the quantised adjacency's own edge list: the dense matrix below holds exactly these
    model = GCNConv_Qnt(F, H, C, w_bit=WB, act_bit=AB, aggr=aggr, float_out=float_out).to(env.dev)
    Wi, Wo = _sparse(np.random.default_rng(7), (F, H), 2.0 ** WB), _sparse(np.random.default_rng(8), (H, C), 2.0 ** WB)
    with torch.no_grad():
        model.W_in.copy_(torch.from_numpy(Wi))
        model.W_out.copy_(torch.from_numpy(Wo))
    Xs = [_sparse(np.random.default_rng(410 + k), (n, F), 2.0 ** AB) for k in range(4)]
    want = [[qnt_model(env.O, s1, d1, n, X, Wi, Wo, aggr, float_out)] for X in Xs]
    buf = torch.empty((n, F), dtype=torch.float32, device=env.dev)
    if adjacency == "dense":
        A = np.zeros((n, n), dtype=np.float32)
        A[s1, d1] = 1.0
        A = torch.from_numpy(A).to(env.dev)
    else:
        A = env.Q.pack_edges_tiled(torch.from_numpy(src).to(env.dev), torch.from_numpy(dst).to(env.dev), n)
    live = sc.Live(torch, [buf], [[X] for X in Xs], want, run=lambda: [model(A, buf)], keep=A)
    with torch.no_grad():
        sc.capture_and_replay(torch, env.Q, live, f"GCNConv_Qnt({adjacency}, {aggr}, float_out={float_out})")
        sc.ordering_probe(torch, env.Q, live, f"GCNConv_Qnt({adjacency}, {aggr}, float_out={float_out})")


def _start(torch, dev):
    from qgtc_ppopp22_amd.conv import GCNConv

    torch.manual_seed(3)
    m = GCNConv(16, 32, 5, norm="sym")
    with torch.no_grad():
        m.W_in.mul_(0.3)
        m.W_out.mul_(0.3)
    m = m.to(dev)
    return m, torch.optim.SGD(m.parameters(), lr=0.5)


def _step(torch, m, opt, adj, X, target):
    opt.zero_grad(set_to_none=True)
    loss = torch.nn.functional.cross_entropy(m(adj, X), target)
    loss.backward()
    opt.step()
    return loss


def test_training_step_under_capture(env):
    """GCNConv(norm="sym") on the self-loop graph of tests/test_tiled_sym_gpu.py: three eager warm-up steps on a side stream, then
    forward + loss + backward + SGD step captured once (torch's whole-network capture recipe). After k replays on the same batch the
    weight bits equal 3 + k eager steps from the same start: the aggregates are functions of their inputs alone and torch.mm is
    run-to-run deterministic on one device (test_training_lowers_the_loss_and_repeats_bit_for_bit relies on the same)."""
    from test_tiled_sym_gpu import _graph_with_loops

    torch, Q, n = env.torch, env.Q, 1200
    _, _, adj = _graph_with_loops(torch, Q, n, 9)
    g = torch.Generator().manual_seed(5)
    X = torch.randn(n, 16, generator=g).to(env.dev)
    target = (X[:, :5] + 0.1 * torch.randn(n, 5, generator=g).to(env.dev)).argmax(dim=1)

    def eager(steps):
        m, opt = _start(torch, env.dev)
        for _ in range(steps):
            _step(torch, m, opt, adj, X, target)
        torch.cuda.synchronize()
        return m.W_in.detach().clone(), m.W_out.detach().clone()

    m, opt = _start(torch, env.dev)
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        for _ in range(3):
            _step(torch, m, opt, adj, X, target)
    cur.wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    opt.zero_grad(set_to_none=True)
    with torch.cuda.graph(graph):
        loss = torch.nn.functional.cross_entropy(m(adj, X), target)
        loss.backward()
        opt.step()
    w3 = eager(3)
    assert torch.equal(m.W_in.detach().view(torch.int32), w3[0].view(torch.int32)), "the capture itself must not run the step"
    for k in (1, 2, 3):
        graph.replay()
        torch.cuda.synchronize()
        want = eager(3 + k)
        assert not torch.equal(want[0], w3[0])
        for name, got, w in (("W_in", m.W_in, want[0]), ("W_out", m.W_out, want[1])):
            assert torch.equal(got.detach().view(torch.int32), w.view(torch.int32)), f"{name} after {k} replays differs from {3 + k} eager steps"
    assert torch.isfinite(loss).all()
