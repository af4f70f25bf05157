"""The multi-head attention entries off the default stream and under graph capture (include/qgtc_attn_heads.h): each ctypes entry takes
the handle of torch's current stream, so behind a head start on a side stream it sees operands a producer wrote on that stream
(tests/stream_cases.py's ordering probe), and a captured graph replays the forward - the max launch and the product - and forward plus
backward - the backward product, the row dot and the two score gradients - on new contents of the operands, three times. The checks are
bit for bit against tests/tiled_attn_heads_model.py. The machine's GPU_MAX_HW_QUEUES is left alone."""
import numpy as np
import pytest

import tiled_attn_heads_model as hm
from stream_cases import Live, empty, graph, warm_adjacency, capture_and_replay, env_of, ordering_probe

pytestmark = pytest.mark.gpu

N_NODES, H, D = 600, 4, 6


def _live(env, transposed, backward):
    torch = env.torch
    n = N_NODES
    src, dst = graph(n, 77)
    adj = warm_adjacency(env, src, dst, n)
    view = adj.T if transposed else adj
    contents, want = [], []
    for k in range(4):
        rng = np.random.default_rng(7700 + k)
        X, G = rng.normal(size=(n, H * D)).astype(np.float32), rng.normal(size=(n, H * D)).astype(np.float32)
        p, q = rng.uniform(-1, 1, (n, H)).astype(np.float32), rng.uniform(-1, 1, (n, H)).astype(np.float32)
        Y, m, inv = hm.attention_heads_f32(src, dst, n, X, p, q, 0.2, transposed)
        contents.append([X, p, q, G])
        if backward:
            want.append([Y, *hm.attention_grads_heads_f32(src, dst, n, X, p, q, G, Y, m, inv, 0.2, transposed)[:3]])
        else:
            want.append([Y, m, inv])
    bufs = [empty(env, (n, H * D), torch.float32), empty(env, (n, H), torch.float32), empty(env, (n, H), torch.float32),
            empty(env, (n, H * D), torch.float32)]
    if backward:
        for b in bufs[:3]:
            b.requires_grad_(True)

        def run():
            y = env.Q.tiledAggregate(view, bufs[0], attn=(bufs[1], bufs[2]))
            return [y.detach(), *torch.autograd.grad(y, bufs[:3], bufs[3])]
    else:
        run = lambda: list(env.Q.tiledMMFloat(view, bufs[0], attn=(bufs[1], bufs[2]), return_stats=True))   # noqa: E731
    return Live(torch, bufs, contents, want, run=run, keep=adj)


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "forward-backward"])
@pytest.mark.parametrize("transposed", [False, True], ids=["adj", "adjT"])
def test_on_a_side_stream_and_under_capture(qgtc, oracle, transposed, backward):
    import torch

    live = _live(env_of(qgtc, oracle, torch), transposed, backward)
    what = f"attention with heads, {'adj.T' if transposed else 'adj'}, {'forward + backward' if backward else 'forward'}"
    ordering_probe(torch, qgtc, live, what)
    capture_and_replay(torch, qgtc, live, what)
