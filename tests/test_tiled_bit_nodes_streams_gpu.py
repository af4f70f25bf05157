"""The masked bit products and the masked quantised layer off the default stream and under graph capture (include/qgtc_bitnodes.h): the
four C entries are reached through ctypes with the handle of torch's current stream, so they must follow it. One ``Live`` case of
tests/stream_cases.py per view and one for ``conv.GCNConv_Qnt.forward(nodes=)``: ``ordering_probe`` puts them behind a timed head start on
three fresh side streams, where they must see the features and the bitmaps a producer wrote on that stream, and ``capture_and_replay``
replays them on three new contents - the features, both bitmaps (read on the device, so a replay follows them) and the induced mean scale
computed from them inside the capture. All checks are bit for bit: the products against tests/tiled_bit_nodes_model.py, the layer
against the same layer on the adjacency packed from the induced edges. The machine's GPU_MAX_HW_QUEUES is left alone."""
import numpy as np
import pytest

import tiled_bit_nodes_model as bn
import tiled_nodes_model as nm
from qgtc_ppopp22_amd.shapes import cols_shape
from stream_cases import Live, capture_and_replay, empty, env_of, ordering_probe, warm_adjacency
from tiled_model import random_edges
from tiled_scaled_model import mean_scale

pytestmark = pytest.mark.gpu

N_COLS = 40


@pytest.fixture(scope="module")
def setup(qgtc, oracle):
    import torch

    env = env_of(qgtc, oracle, torch)
    n = 600
    rng = np.random.default_rng(47)
    src, dst = (np.asarray(a, dtype=np.int64) for a in random_edges(rng, n, 6 * n + 5))
    adj = warm_adjacency(env, src, dst, n)
    return env, n, src, dst, adj


def _products_live(env, transposed, n, src, dst, adj):
    """tiledMM2Bit and tiledMM2Int under both masks, as the plain sum and under the induced mean scale: four contents that differ in the
    features and in both bitmaps"""
    torch, Q = env.torch, env.Q
    bit2, ob = bn.BITS
    a = adj.T if transposed else adj
    rng = np.random.default_rng(48 + transposed)
    contents, wants = [], []
    for _ in range(4):
        Xq = rng.integers(0, 2 ** bit2, size=(n, N_COLS))
        R, S = rng.random(n) < 0.5, rng.random(n) < 0.5
        C = bn.sums(src, dst, n, Xq, R, S, transposed)
        deg = bn.sums(src, dst, n, np.ones((n, 1), np.int64), R, S, transposed)[:, 0]
        want = []
        for scale in (None, mean_scale(deg)):
            floats, bits = bn.reference(env.O, C, ob, scale)
            want += [bits.view(np.int32), floats]
        contents.append([env.O.pack(Xq, bit2, True), nm.bitmap(R), nm.bitmap(S)])
        wants.append(want)
    X = empty(env, cols_shape(n, N_COLS, bit2), torch.int32)
    rm, sm = empty(env, (adj.mask_words,), torch.int32), empty(env, (adj.mask_words,), torch.int32)

    def run():
        ms = a.mean_scale(row_mask=rm, nbr_mask=sm)
        return [Q.tiledMM2Bit(a, X, N_COLS, bit2, ob, row_mask=rm, nbr_mask=sm).reshape(-1),
                Q.tiledMM2Int(a, X, N_COLS, bit2, row_mask=rm, nbr_mask=sm),
                Q.tiledMM2Bit(a, X, N_COLS, bit2, ob, ms, row_mask=rm, nbr_mask=sm).reshape(-1),
                Q.tiledMM2Int(a, X, N_COLS, bit2, ms, row_mask=rm, nbr_mask=sm)]

    return Live(torch, [X, rm, sm], contents, wants, run=run, keep=adj)


@pytest.mark.parametrize("transposed", [False, True], ids=["adj", "adjT"])
def test_the_masked_products_on_a_side_stream_and_under_capture(setup, transposed):
    env = setup[0]
    live = _products_live(env, transposed, *setup[1:])
    what = f"masked bit products, {'adj.T' if transposed else 'adj'}"
    ordering_probe(env.torch, env.Q, live, what)
    capture_and_replay(env.torch, env.Q, live, what)


def _layer_live(env, transposed, n, src, dst, adj):
    """conv.GCNConv_Qnt(aggr="mean").forward(nodes=): four contents that differ in X and in the node set; the reference is the layer on
    the adjacency packed from the induced edges, computed on the default stream before any probe"""
    torch, Q = env.torch, env.Q
    from qgtc_ppopp22_amd import conv

    F_in, H, C = 12, 20, 7
    a = adj.T if transposed else adj
    rng = np.random.default_rng(50 + transposed)
    torch.manual_seed(0)
    layer = conv.GCNConv_Qnt(F_in, H, C, aggr="mean").to(env.dev)
    contents, wants = [], []
    for _ in range(4):
        Xh = rng.uniform(0.0, 8.0, (n, F_in)).astype(np.float32)
        nodes = rng.random(n) < 0.5
        ks, kd = nm.induced_edges(src, dst, n, nodes, nodes, False)
        kadj = Q.pack_edges_tiled(torch.from_numpy(ks).to(env.dev), torch.from_numpy(kd).to(env.dev), n)
        with torch.no_grad():
            wants.append([layer(kadj.T if transposed else kadj, torch.from_numpy(Xh).to(env.dev)).cpu()])
        contents.append([Xh, nodes])
    X, flags = empty(env, (n, F_in), torch.float32), empty(env, (n,), torch.bool)

    def run():
        with torch.no_grad():
            return [layer(a, X, nodes=flags)]

    return Live(torch, [X, flags], contents, wants, run=run, keep=(adj, layer))


@pytest.mark.parametrize("transposed", [False, True], ids=["adj", "adjT"])
def test_the_masked_layer_on_a_side_stream_and_under_capture(setup, transposed):
    env = setup[0]
    live = _layer_live(env, transposed, *setup[1:])
    what = f"GCNConv_Qnt(nodes=), {'adj.T' if transposed else 'adj'}"
    ordering_probe(env.torch, env.Q, live, what)
    capture_and_replay(env.torch, env.Q, live, what)
