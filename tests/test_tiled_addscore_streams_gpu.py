"""The additive-score entries off the default stream and under graph capture (include/qgtc_addscore.h: the score and its gradient folds
on both views): each ctypes entry takes the handle of torch's current stream. One ``Live`` case of tests/stream_cases.py per view:
``ordering_probe`` puts every entry - alone and composed into the GATv2 attention with its four gradients - behind a timed head start on
three fresh side streams, where it must see operands a producer wrote on that stream, and ``capture_and_replay`` replays them on three
new contents of the operands. The checks are bit for bit against the model of tests/tiled_addscore_model.py. The machine's
GPU_MAX_HW_QUEUES is left alone."""
import numpy as np
import pytest

import tiled_addscore_model as am
import tiled_edge_model as em
from stream_cases import Live, capture_and_replay, empty, env_of, ordering_probe, warm_adjacency
from tiled_model import random_edges

pytestmark = pytest.mark.gpu

H, D, DV = 4, 6, 10   # own and nbr are [n, 24], V is [n, 40]
SLOPE = 0.2


def _live(env, transposed):
    from qgtc_ppopp22_amd import tiled

    torch = env.torch
    n = 300
    rng = np.random.default_rng(6)
    src, dst = (np.asarray(a, dtype=np.int64) for a in random_edges(rng, n, 6 * n))
    adj = warm_adjacency(env, src, dst, n)
    a = adj.T if transposed else adj
    nnz = em.slot_cells(src, dst, n)[0].size
    data = [(rng.normal(size=(nnz, H)).astype(np.float32), rng.normal(size=(n, H * D)).astype(np.float32),
             rng.normal(size=(n, H * D)).astype(np.float32), rng.normal(size=(H, D)).astype(np.float32),
             rng.normal(size=(n, H * DV)).astype(np.float32), rng.normal(size=(n, H * DV)).astype(np.float32))
            for _ in range(4)]   # (g, own, nbr, att, V, dY)
    g, own, nbr, att, V, dY = bufs = [empty(env, t.shape, torch.float32) for t in data[0]]

    def run():
        s = tiled.tiledEdgeAdditiveScores(a, own, nbr, att, SLOPE, heads=H)           # the score entry
        d_own, P = tiled._addscore_grad(a, own, nbr, att, SLOPE, g, H, True, True)     # the gradient entry of this view, both outputs
        d_nbr, _ = tiled._addscore_grad(a.T, nbr, own, att, SLOPE, g, H, True, False)  # and of the other, one output
        leaves = [t.clone().requires_grad_(True) for t in (own, nbr, V, att)]
        Y = tiled.tiledEdgeAdditiveAttention(a, leaves[0], leaves[1], leaves[2], leaves[3], SLOPE, heads=H)
        go, gn, gV, ga = torch.autograd.grad(Y, leaves, dY)
        return [s, d_own, P, d_nbr, Y.detach(), go, gn, gV, ga]

    def want(c):
        gn, on, nn, an, Vn, dYn = c
        d_own, P = am.addscore_grad_heads_f32(src, dst, n, on, nn, an, SLOPE, gn, H, transposed)
        d_nbr, _ = am.addscore_grad_heads_f32(src, dst, n, nn, on, an, SLOPE, gn, H, not transposed)
        w_own, w_nbr, w_V, w_P = am.additive_attention_grads_heads_f32(src, dst, n, on, nn, Vn, an, SLOPE, H, dYn, transposed)
        return [am.addscore_heads_f32(src, dst, n, on, nn, an, SLOPE, H, transposed), d_own, P, d_nbr,
                am.additive_attention_heads_f32(src, dst, n, on, nn, Vn, an, SLOPE, H, transposed)[0], w_own, w_nbr, w_V,
                torch.from_numpy(np.ascontiguousarray(w_P)).to(env.dev).sum(dim=0).view(H, D).cpu().numpy()]   # att's gradient: torch's reduction of the model's P

    return Live(torch, bufs, data, [[np.asarray(w, dtype=np.float32) for w in want(c)] for c in data], run=run, keep=adj)


@pytest.mark.parametrize("transposed", [False, True])
def test_every_entry_on_a_side_stream_and_under_capture(qgtc, oracle, transposed):
    import torch

    live = _live(env_of(qgtc, oracle, torch), transposed)
    what = f"the additive-score entries, {'adj.T' if transposed else 'adj'}"
    ordering_probe(torch, qgtc, live, what)
    capture_and_replay(torch, qgtc, live, what)
