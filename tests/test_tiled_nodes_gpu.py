"""Node masks on the device (``row_mask=`` / ``nbr_mask=`` of QGTC.tiledMMFloat / QGTC.tiledAggregate, tiled.node_bitmap, the masked
degrees, ``nodes=`` of conv.GCNConv / conv.GATConv and the C-ABI _nodes entries) against tests/tiled_nodes_model.py: masking is
restricting the edge list, so every masked operator must give, bit for bit, what the exact models give on the induced edges and what the
unmasked operator gives on ``pack_edges_tiled`` of the induced edges. Nothing is sampled and no tolerance is used."""
import ctypes

import numpy as np
import pytest

import tiled_nodes_model as nm
from qgtc_ppopp22_amd.tiled import node_bitmap
from stream_cases import Live, capture_and_replay, eager_results, empty, env_of, ordering_probe, warm_adjacency
from test_tiled_drop_gpu import NAMES, _assert_all, _dev, _forwards, _grads, _inputs, _models, _np, _same
from test_tiled_float_gpu import CANARY, NAN_WORD, NO_EDGES, assert_floats_identical
from tiled_attn_model import (ATT_FORWARD_VARIANTS, ATT_GRAD_VARIANTS, ATT_TRANSPOSED_VARIANTS, att_grad_variant, att_variant, attention_f32,
                              attention_grads_f32, lrelu_f32)
from tiled_float_model import FLOAT_FORWARD_VARIANTS, FLOAT_TRANSPOSED_VARIANTS, float_variant, neighbour_lists
from tiled_max_model import MAX, MAX_FORWARD_VARIANTS, MAX_TRANSPOSED_VARIANTS, extremum_f32, max_variant, select_f32
from tiled_model import random_edges
from tiled_scaled_model import mean_scale
from tiled_sym_model import aggregate_f32_src, inv_sqrt_degree

pytestmark = pytest.mark.gpu

SWEEP_N = (1, 16, 17, 33, 65, 129, 257)
SWEEP_n = (97, 333, 1000)                          # n % 32 and n % 128 are nonzero
KINDS = ("both", "rows", "nbrs", "same")           # (random, random), (random, none), (none, random), one mask twice
# the grid N x n x both views x mask pair, thinned as the edge-dropout sweep is: every (n, N) runs both views under one pair, which rotates
SWEEP = [(n, N, KINDS[(iN + i) % 4]) for iN, N in enumerate(SWEEP_N) for i, n in enumerate(SWEEP_n)]


def _pair(rng, n, kind):
    """(R, S) bool [n] or None each, of density 0.5"""
    a, b = rng.random(n) < 0.5, rng.random(n) < 0.5
    return {"both": (a, b), "rows": (a, None), "nbrs": (None, b), "same": (a, a)}[kind]


def _bm(torch, qgtc, flags, n):
    return None if flags is None else node_bitmap(_dev(torch, flags), n)


def _kw(torch, qgtc, R, S, n):
    return {"row_mask": _bm(torch, qgtc, R, n), "nbr_mask": _bm(torch, qgtc, S, n)}


def _check(torch, qgtc, src, dst, n, N, R, S, rng, what, adj=None, repack=True):
    """both views under (R, S), which are relative to the view: the masked operators on `adj` against the models on the induced edges
    and, with `repack`, against the unmasked operators on the adjacency packed from the induced edges; the three attention gradients too"""
    X, dY, p, q, r, c = _inputs(rng, n, N)
    adj = adj if adj is not None else qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    kw = _kw(torch, qgtc, R, S, n)
    for transposed in (False, True):
        a = adj.T if transposed else adj
        ks, kd = nm.induced_edges(src, dst, n, R, S, transposed)
        w = f"{what} {'adj.T' if transposed else 'adj'}"
        got = _forwards(torch, qgtc, a, X, p, q, r, c, **kw)
        _assert_all(got, _models(ks, kd, n, X, p, q, r, c, transposed), w + " against the model")
        if repack:
            kadj = qgtc.pack_edges_tiled(_dev(torch, ks), _dev(torch, kd), n)
            _assert_all(got, _forwards(torch, qgtc, kadj.T if transposed else kadj, X, p, q, r, c), w + " against the re-packed adjacency")
        Y, m, inv = got[8:]
        want = attention_grads_f32(ks, kd, n, X, p, q, dY, Y, m, inv, 0.2, transposed)[:3]
        for name, g, wv in zip(("dX", "dp", "dq"), _grads(torch, qgtc, a, X, dY, p, q, r, c, "attn", **kw)[1:], want):
            assert_floats_identical(g, wv, f"{w} attention {name}")
        if R is not None:                          # rows outside the row mask: +0, arg -1, inv 0, m = L(p)
            out = ~R
            for name, g in zip(NAMES, got):
                if name in ("argmax", "argmin"):
                    assert (g[out] == -1).all(), name
                elif name == "m":
                    assert_floats_identical(g[out], lrelu_f32(p[out], 0.2), "m of a masked-out row is L(p)")
                else:
                    assert (g[out].view(np.uint32) == 0).all(), name      # +0 (times a positive row scale), and inv = 0
    return adj, (X, dY, p, q, r, c)


def _filled_edges(rng, n, e):
    """random_edges (hubs, loops, duplicates) plus uniform edges, so that no row block or k-quad is left empty"""
    src, dst = random_edges(rng, n, e)
    return (np.concatenate([src, rng.integers(0, n, size=e, dtype=np.int64)]),
            np.concatenate([dst, rng.integers(0, n, size=e, dtype=np.int64)]))


# ---- 1. the sweep ---------------------------------------------------------------------------------------------------------------------------
def test_the_sweep_reaches_every_launcher_variant():
    """Against the models' copies of the launchers' switches: the entries of qgtc_tiled_float_nodes.hip,
    qgtc_tiled_float_t_nodes.hip, qgtc_tiled_max_nodes.hip, qgtc_tiled_attn_nodes.hip and qgtc_tiled_attn_t_nodes.hip go through their
    parents' launchers (one per kernel family, at the foot of its tiled_*_kernels.hip.h), so they choose as their parents do. Every case runs
    the plain sum, each scale alone and both (all four packs of the float kernels), max and min with arg, the
    attention forward and its three gradients, on both views."""
    for transposed, fl, mx, at in ((False, FLOAT_FORWARD_VARIANTS, MAX_FORWARD_VARIANTS, ATT_FORWARD_VARIANTS),
                                   (True, FLOAT_TRANSPOSED_VARIANTS, MAX_TRANSPOSED_VARIANTS, ATT_TRANSPOSED_VARIANTS)):
        assert sorted({float_variant(N, transposed) for N in SWEEP_N}) == sorted(fl)
        assert sorted({max_variant(N, transposed) for N in SWEEP_N}) == sorted(mx)
        assert sorted({att_variant(N, transposed) for N in SWEEP_N}) == sorted(at)
    assert sorted({att_grad_variant(N) for N in SWEEP_N}) == sorted(ATT_GRAD_VARIANTS)
    assert len(SWEEP) == 21 and {s[0] for s in SWEEP} == set(SWEEP_n) and {s[1] for s in SWEEP} == set(SWEEP_N)
    for kind in KINDS:                             # every pair meets every n, and a narrow, a middle and a wide output
        assert {s[0] for s in SWEEP if s[2] == kind} == set(SWEEP_n)
        assert len({s[1] for s in SWEEP if s[2] == kind}) >= 5
    for N in SWEEP_N:                              # every output width runs under three of the four pairs
        assert len({s[2] for s in SWEEP if s[1] == N}) == 3


@pytest.mark.parametrize("n,N,kind", SWEEP, ids=[f"n{n}-N{N}-{k}" for n, N, k in SWEEP])
def test_masked_operators_equal_the_model_and_the_repacked_adjacency(qgtc, n, N, kind):
    import torch

    rng = np.random.default_rng(17 * n + N)
    src, dst = random_edges(rng, n, 6 * n + 5)
    R, S = _pair(rng, n, kind)
    _check(torch, qgtc, src, dst, n, N, R, S, rng, f"n={n} N={N} {kind}")


# ---- 2. the edges of the mask -----------------------------------------------------------------------------------------------------------------
def _between(n, lo, hi):
    f = np.zeros(n, bool)
    f[lo:hi] = True
    return f


EDGE_MASKS = {
    "empty": lambda n: np.zeros(n, bool),
    "one node": lambda n: _between(n, 70, 71),
    "one row block": lambda n: _between(n, 32, 64),
    "one k-quad": lambda n: _between(n, 128, 256),
    "the last node": lambda n: _between(n, n - 1, n),
}


@pytest.mark.parametrize("which", sorted(EDGE_MASKS))
def test_edge_masks(qgtc, which):
    """Each special set as the row mask alone, as the neighbour mask alone (under a random other mask), and as both."""
    import torch

    n, N = 333, 33
    rng = np.random.default_rng(len(which))
    src, dst = _filled_edges(rng, n, 4 * n)
    f = EDGE_MASKS[which](n)
    other = rng.random(n) < 0.5
    adj = None
    for R, S in ((f, None), (None, f), (f, other), (other, f), (f, f)):
        adj, _ = _check(torch, qgtc, src, dst, n, N, R, S, rng, which, adj=adj)


def test_all_ones_masks_give_the_plain_bits(qgtc):
    import torch

    n, N = 333, 70
    rng = np.random.default_rng(2)
    src, dst = random_edges(rng, n, 6 * n + 5)
    X, dY, p, q, r, c = _inputs(rng, n, N)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    ones = np.ones(n, bool)
    for a in (adj, adj.T):
        plain = _forwards(torch, qgtc, a, X, p, q, r, c)
        for R, S in ((ones, ones), (ones, None), (None, ones), (None, None)):
            _assert_all(_forwards(torch, qgtc, a, X, p, q, r, c, **_kw(torch, qgtc, R, S, n)), plain, "all ones")
        for mode in ("sym", "max", "attn"):
            want = _grads(torch, qgtc, a, X, dY, p, q, r, c, mode)
            got = _grads(torch, qgtc, a, X, dY, p, q, r, c, mode, **_kw(torch, qgtc, ones, ones, n))
            for g, w in zip(got, want):
                assert (g is None) == (w is None)
                if g is not None:
                    assert_floats_identical(g, w, mode)


@pytest.mark.parametrize("n,N,loop", [(1, 1, False), (1, 5, True), (300, 24, False)])
def test_one_node_and_an_empty_adjacency(qgtc, n, N, loop):
    import torch

    rng = np.random.default_rng(n + N)
    src, dst = (np.zeros(1, np.int64), np.zeros(1, np.int64)) if loop else NO_EDGES
    for R, S in ((np.ones(n, bool), np.ones(n, bool)), (np.zeros(n, bool), None), (None, np.zeros(n, bool))):
        _check(torch, qgtc, src, dst, n, N, R, S, rng, f"n={n} loop={loop}")


def test_node_4096_of_4097(qgtc):
    """n = 4097: node 4096 is alone in the last row block and the last k-quad, whose other 127 bitmap bits are pad."""
    import torch

    n, N = 4097, 3
    rng = np.random.default_rng(4097)
    src, dst = random_edges(rng, n, 2 * n)
    last = np.full(40, n - 1, np.int64)
    far = rng.integers(0, n, size=40, dtype=np.int64)
    src, dst = np.concatenate([src, last, far, [n - 1]]), np.concatenate([dst, far, last, [n - 1]])
    f = _between(n, n - 1, n)
    other = rng.random(n) < 0.5
    other[n - 1] = True
    adj = None
    for R, S in ((f, None), (None, f), (other, other)):
        adj, _ = _check(torch, qgtc, src, dst, n, N, R, S, rng, "n=4097", adj=adj)


# ---- 3. other device cases --------------------------------------------------------------------------------------------------------------------
def test_nan_outside_the_masks_reaches_nothing(qgtc):
    """NaN in every row of X (and every score) outside nbr_mask: no output of a computed row sees one, in any mode. Rows outside row_mask
    are +0 even though all their neighbours are NaN."""
    import torch

    n, N = 333, 40
    rng = np.random.default_rng(9)
    src, dst = random_edges(rng, n, 6 * n + 5)
    X, dY, p, q, r, c = _inputs(rng, n, N)
    R, S = rng.random(n) < 0.5, rng.random(n) < 0.5
    Xn, qn, cn = X.copy(), q.copy(), c.copy()
    Xn[~S], qn[~S], cn[~S] = np.nan, np.nan, np.nan
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    kw = _kw(torch, qgtc, R, S, n)
    for a in (adj, adj.T):
        clean = _forwards(torch, qgtc, a, X, p, q, r, c, **kw)
        dirty = _forwards(torch, qgtc, a, Xn, p, qn, r, cn, **kw)
        for name, g, w in zip(NAMES, dirty, clean):
            assert not np.isnan(g).any(), name
            assert (g.view(np.uint32) == w.view(np.uint32)).all(), name
        # all of X NaN: rows outside the row mask still hold +0
        allnan = _forwards(torch, qgtc, a, np.full_like(X, np.nan), p, q, np.ones_like(r), c, **kw)
        for name, g in zip(NAMES, allnan):
            if name in ("sum", "row scale", "both scales", "source scale", "max", "min", "attention"):
                assert (g[~R].view(np.uint32) == 0).all(), name


def test_a_hub_keeps_more_than_a_queue(qgtc):
    """Hub h has 300 out-edges and 300 in-edges at n = 600; under masks of density 0.5 more than 32 of each take part, so its queue
    flushes mid-row with masked-out neighbours in between; and the hub's k-quad lists more than 8 tiles, so the column view stages it in
    several rounds."""
    import torch

    n, h, N = 600, 301, 40
    rng = np.random.default_rng(4)
    others = rng.permutation(np.delete(np.arange(n, dtype=np.int64), h))[:300]
    extra = random_edges(rng, n, 2 * n)
    keep = (extra[0] != h) & (extra[1] != h)
    src = np.concatenate([np.full(300, h, np.int64), others, extra[0][keep]])
    dst = np.concatenate([others, np.full(300, h, np.int64), extra[1][keep]])
    R, S = rng.random(n) < 0.5, rng.random(n) < 0.5
    R[h] = S[h] = True
    for transposed in (False, True):
        ks, kd = nm.induced_edges(src, dst, n, R, S, transposed)
        part = int(((kd if transposed else ks) == h).sum())
        assert 32 < part < 300, part
    adj, _ = _check(torch, qgtc, src, dst, n, N, R, S, rng, "hub")
    assert adj.T.max_block_tiles > 8


def test_two_launches_agree_and_two_masks_differ(qgtc):
    import torch

    n, N = 1000, 96
    rng = np.random.default_rng(6)
    src, dst = random_edges(rng, n, 6 * n + 5)
    X, dY, p, q, r, c = _inputs(rng, n, N)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    R, S, S2 = rng.random(n) < 0.5, rng.random(n) < 0.5, rng.random(n) < 0.5
    for a in (adj, adj.T):
        first, again, other = (_forwards(torch, qgtc, a, X, p, q, r, c, **_kw(torch, qgtc, R, s, n)) for s in (S, S, S2))
        for name, f, g, o in zip(NAMES, first, again, other):
            assert (f.view(np.uint32) == g.view(np.uint32)).all(), name
            if name != "m":                        # m = L(p + max q) may coincide row by row; everything else differs somewhere
                assert (f.view(np.uint32) != o.view(np.uint32)).any(), name


def _live(env, transposed):
    """Masked forward and backward of all three modes as a ``Live`` case of tests/stream_cases.py: X, dY, p and q are the contents, one
    pair of scales and one pair of bitmaps stay; the reference is the eager result on the default stream."""
    torch, qgtc = env.torch, env.Q
    n, N = 600, 40
    rng = np.random.default_rng(41)
    src, dst = random_edges(rng, n, 6 * n + 5)
    adj = warm_adjacency(env, src, dst, n)
    a = adj.T if transposed else adj
    data = [_inputs(rng, n, N) for _ in range(4)]      # (X, dY, p, q, r, c)
    Rf, Sf = rng.random(n) < 0.5, rng.random(n) < 0.5
    kw = {"row_mask": _bm(torch, qgtc, Rf, n), "nbr_mask": _bm(torch, qgtc, Sf, n)}
    r, c = _dev(torch, data[0][4]), _dev(torch, data[0][5])
    contents = [d[:4] for d in data]
    X, dY, p, q = bufs = [empty(env, t.shape, torch.float32) for t in contents[0]]
    for t in (X, p, q):
        t.requires_grad_(True)

    def run():
        Ys = qgtc.tiledAggregate(a, X, r, c, **kw)
        Ym = qgtc.tiledAggregate(a, X, reduce="max", **kw)
        Ya = qgtc.tiledAggregate(a, X, attn=(p, q), **kw)
        grads = torch.autograd.grad(Ys, X, dY) + torch.autograd.grad(Ym, X, dY) + torch.autograd.grad(Ya, (X, p, q), dY)
        return [Ys.detach(), Ym.detach(), Ya.detach(), *grads]

    return Live(torch, bufs, contents, eager_results(torch, bufs, contents, run), run=run, keep=(adj, kw))


@pytest.mark.parametrize("transposed", [False, True], ids=["adj", "adjT"])
def test_side_stream_and_graph_capture(qgtc, oracle, transposed):
    """Masked forward and backward of all three modes behind a timed head start on three fresh side streams (``ordering_probe``) and
    captured into a graph; three replays on new inputs equal the eager results (``capture_and_replay``)."""
    import torch

    live = _live(env_of(qgtc, oracle, torch), transposed)
    what = f"node masks, {'adj.T' if transposed else 'adj'}"
    ordering_probe(torch, qgtc, live, what)
    capture_and_replay(torch, qgtc, live, what)


# ---- 4. the C entries write what they own and nothing else, and ignore pad bits ----------------------------------------------------------------
@pytest.mark.parametrize("n,N", [(97, 17), (333, 129)])
def test_the_c_entries_stay_within_their_outputs_and_ignore_pad_bits(qgtc, n, N):
    """Every _nodes entry through ctypes, into NaN-filled outputs with canaries behind them, from HAND-MADE bitmaps whose pad bits (the
    positions from n up) are all set: the outputs are the models' on the induced edges."""
    import torch

    from qgtc_ppopp22_amd import cabi

    L = cabi.load()
    rng = np.random.default_rng(n)
    src, dst = random_edges(rng, n, 6 * n + 5)
    X, dY, p, q, r, c = _inputs(rng, n, N)
    Rf, Sf = rng.random(n) < 0.5, rng.random(n) < 0.5
    words = nm.bitmap_words(n)

    def dirty(flags):
        """the bitmap with every pad bit set, as a device tensor"""
        padded = np.ones(words * 32, bool)
        padded[:n] = flags
        w = nm.bitmap(padded)
        assert (nm.members(w, n) == flags).all() and (w != nm.bitmap(flags)).any()
        return _dev(torch, w.view(np.int32))

    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    dX_, ddY, dp_, dq_, dr_, dc_ = (_dev(torch, t) for t in (X, dY, p, q, r, c))
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fresh(elems, dtype=torch.float32):
        if dtype == torch.int32:
            return torch.full((elems + CANARY,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        return torch.full((elems + CANARY,), float("nan"), dtype=torch.float32, device="cuda")

    def taken(buf, elems):
        a = buf.cpu().numpy()
        assert (a[elems:].view(np.uint32) == (0x5A5A5A5A if a.dtype == np.int32 else NAN_WORD)).all(), "canaries"
        return a[:elems]

    for transposed in (False, True):
        t = adj.T
        idx = (t.col_ptr.data_ptr(), t.col_tile.data_ptr(), t.col_rb.data_ptr(), adj.tiles.data_ptr()) if transposed else \
            (adj.row_ptr.data_ptr(), adj.kquad.data_ptr(), adj.tiles.data_ptr())
        sfx = "_t_nodes" if transposed else "_nodes"
        rm, sm = dirty(Rf), dirty(Sf)
        here = (rm.data_ptr(), sm.data_ptr(), words)      # the masks of a forward on this view
        swapped = (sm.data_ptr(), rm.data_ptr(), words)   # ... and of the launches of a forward on the OTHER view that run on this one
        ks, kd = nm.induced_edges(src, dst, n, Rf, Sf, transposed)
        want = dict(zip(NAMES, _models(ks, kd, n, X, p, q, r, c, transposed)))
        for name, rs, cs in (("sum", None, None), ("row scale", dr_, None), ("both scales", dr_, dc_), ("source scale", None, dc_)):
            out = fresh(n * N)
            rc = getattr(L, "qgtc_tiledmm_f32" + sfx)(*idx, adj.n_tiles, n, dX_.data_ptr(), n * N, N, rs.data_ptr() if rs is not None else None,
                                                      cs.data_ptr() if cs is not None else None, out.data_ptr(), n * N, *here, st)
            assert rc == 0
            assert_floats_identical(taken(out, n * N).reshape(n, N), want[name], "C " + name)
        out = fresh(n * N)                         # one mask alone, and none: a NULL is all nodes
        rc = getattr(L, "qgtc_tiledmm_f32" + sfx)(*idx, adj.n_tiles, n, dX_.data_ptr(), n * N, N, None, None, out.data_ptr(), n * N,
                                                  rm.data_ptr(), None, words, st)
        assert rc == 0
        ro = nm.induced_edges(src, dst, n, Rf, None, transposed)
        assert_floats_identical(taken(out, n * N).reshape(n, N), aggregate_f32_src(*ro, n, X, transposed), "C row mask alone")
        out = fresh(n * N)
        rc = getattr(L, "qgtc_tiledmm_f32" + sfx)(*idx, adj.n_tiles, n, dX_.data_ptr(), n * N, N, None, None, out.data_ptr(), n * N, None,
                                                  None, 0, st)
        assert rc == 0
        assert_floats_identical(taken(out, n * N).reshape(n, N), aggregate_f32_src(src, dst, n, X, transposed), "C no masks")
        for op, name in ((0, "max"), (1, "min")):
            out, arg = fresh(n * N), fresh(n * N, torch.int32)
            rc = getattr(L, "qgtc_tiledmax_f32" + sfx)(*idx, adj.n_tiles, n, dX_.data_ptr(), n * N, N, op, out.data_ptr(), n * N, arg.data_ptr(),
                                                       n * N, *here, st)
            assert rc == 0
            assert_floats_identical(taken(out, n * N).reshape(n, N), want[name], "C " + name)
            np.testing.assert_array_equal(taken(arg, n * N).reshape(n, N), want["arg" + name])
            out = fresh(n * N)                    # without arg
            rc = getattr(L, "qgtc_tiledmax_f32" + sfx)(*idx, adj.n_tiles, n, dX_.data_ptr(), n * N, N, op, out.data_ptr(), n * N, None, 0,
                                                       *here, st)
            assert rc == 0
            assert_floats_identical(taken(out, n * N).reshape(n, N), want[name], "C " + name + " without arg")
        # the attention forward from the MASKED maximum of the neighbours' scores
        M = fresh(n)
        rc = getattr(L, "qgtc_tiledmax_f32" + sfx)(*idx, adj.n_tiles, n, dq_.data_ptr(), n, 1, 0, M.data_ptr(), n, None, 0, *here, st)
        assert rc == 0
        taken(M, n)
        Y, m, inv = want["attention"], want["m"], want["inv"]
        out, mo, io = fresh(n * N), fresh(n), fresh(n)
        rc = getattr(L, "qgtc_tiledatt_f32" + sfx)(*idx, adj.n_tiles, n, dX_.data_ptr(), n * N, N, dp_.data_ptr(), dq_.data_ptr(), 0.2, 0,
                                                   M.data_ptr(), mo.data_ptr(), io.data_ptr(), out.data_ptr(), n * N, *here, st)
        assert rc == 0
        assert_floats_identical(taken(out, n * N).reshape(n, N), Y, "C forward")
        assert_floats_identical(taken(mo, n), m, "C m")
        assert_floats_identical(taken(io, n), inv, "C inv")
        gX, gp, gq, Dm = attention_grads_f32(ks, kd, n, X, p, q, dY, Y, m, inv, 0.2, transposed)
        dm_, di_, D = _dev(torch, m), _dev(torch, inv), _dev(torch, Dm)
        g = fresh(n)
        rc = getattr(L, "qgtc_tiledatt_grad_f32" + sfx)(*idx, adj.n_tiles, n, ddY.data_ptr(), dX_.data_ptr(), n * N, N, dp_.data_ptr(),
                                                        dq_.data_ptr(), 0.2, 0, dm_.data_ptr(), di_.data_ptr(), D.data_ptr(), g.data_ptr(), n,
                                                        *here, st)
        assert rc == 0
        assert_floats_identical(taken(g, n), gp, "C dp")
        # the other two gradients of the forward on the OTHER view (under Rf, Sf there) run on this one with the masks swapped
        ko = nm.induced_edges(src, dst, n, Rf, Sf, not transposed)
        Yo, m_o, inv_o = attention_f32(*ko, n, X, p, q, 0.2, not transposed)
        gXo, _, gqo, Do = attention_grads_f32(*ko, n, X, p, q, dY, Yo, m_o, inv_o, 0.2, not transposed)
        dmo, dio, Dod = _dev(torch, m_o), _dev(torch, inv_o), _dev(torch, Do)
        out = fresh(n * N)
        rc = getattr(L, "qgtc_tiledatt_f32" + sfx)(*idx, adj.n_tiles, n, ddY.data_ptr(), n * N, N, dq_.data_ptr(), dp_.data_ptr(), 0.2, 1,
                                                   dmo.data_ptr(), None, dio.data_ptr(), out.data_ptr(), n * N, *swapped, st)
        assert rc == 0
        assert_floats_identical(taken(out, n * N).reshape(n, N), gXo, "C dX")
        g = fresh(n)
        rc = getattr(L, "qgtc_tiledatt_grad_f32" + sfx)(*idx, adj.n_tiles, n, dX_.data_ptr(), ddY.data_ptr(), n * N, N, dq_.data_ptr(),
                                                        dp_.data_ptr(), 0.2, 1, dmo.data_ptr(), dio.data_ptr(), Dod.data_ptr(), g.data_ptr(), n,
                                                        *swapped, st)
        assert rc == 0
        assert_floats_identical(taken(g, n), gqo, "C dq")
    torch.cuda.synchronize()


# ---- 5. autograd ------------------------------------------------------------------------------------------------------------------------------
def _grad_models(ks, kd, n, X, dY, p, q, r, c, mode, transposed):
    """[Y, dX, dp, dq] of tiledAggregate in `mode` on the edge list (ks, kd), by the exact models"""
    if mode == "sym":
        return [aggregate_f32_src(ks, kd, n, X, transposed, r, c), aggregate_f32_src(ks, kd, n, dY, not transposed, c, r), None, None]
    if mode == "max":
        Y, arg = extremum_f32(ks, kd, n, X, transposed, MAX)
        return [Y, select_f32(ks, kd, n, dY, arg, not transposed), None, None]
    Y, m, inv = attention_f32(ks, kd, n, X, p, q, 0.2, transposed)
    return [Y] + list(attention_grads_f32(ks, kd, n, X, p, q, dY, Y, m, inv, 0.2, transposed)[:3])


@pytest.mark.parametrize("mode", ["sym", "max", "attn"])
def test_backward_equals_the_models_on_the_induced_edges(qgtc, mode):
    """X.grad (and both score gradients) under independent masks, on adj, on adj.T and on a reordered adjacency, against the models on
    the induced edges and against the unmasked composition on the re-packed adjacency. The backward takes the masks swapped: with them
    unswapped these gradients differ (tests/test_tiled_nodes_model.py: the swapped rule changes at least half the rows)."""
    import torch

    n, N = 333, 70
    rng = np.random.default_rng(5)
    src, dst = random_edges(rng, n, 6 * n + 5)
    X, dY, p, q, r, c = _inputs(rng, n, N)
    R, S = rng.random(n) < 0.5, rng.random(n) < 0.5
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    kw = _kw(torch, qgtc, R, S, n)
    needs = (True, True, True) if mode == "attn" else (True, False, False)
    for transposed in (False, True):
        a = adj.T if transposed else adj
        ks, kd = nm.induced_edges(src, dst, n, R, S, transposed)
        kadj = qgtc.pack_edges_tiled(_dev(torch, ks), _dev(torch, kd), n)
        got = _grads(torch, qgtc, a, X, dY, p, q, r, c, mode, needs, **kw)
        want = _grads(torch, qgtc, kadj.T if transposed else kadj, X, dY, p, q, r, c, mode, needs)
        plain = _grads(torch, qgtc, a, X, dY, p, q, r, c, mode, needs)
        model = _grad_models(ks, kd, n, X, dY, p, q, r, c, mode, transposed)
        for k, (g, w, u, mdl) in enumerate(zip(got, want, plain, model)):
            assert (g is None) == (w is None) == (mdl is None), (mode, k)
            if g is not None:
                assert_floats_identical(g, w, f"{mode} output {k} transposed={transposed} against the re-packed adjacency")
                assert_floats_identical(g, mdl, f"{mode} output {k} transposed={transposed} against the model")
                assert (g.view(np.uint32) != u.view(np.uint32)).any(), "the masks change the result"
        assert (got[1][~S].view(np.uint32) == 0).all()         # a neighbour outside nbr_mask gets no gradient: +0
    # a reordered adjacency: masks and edges in the NEW numbering
    re = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n, reorder=True)
    rank = re.rank.cpu().numpy()
    assert (rank != np.arange(n)).any()
    Rn, Sn = _np(re.to_new(_dev(torch, R))), _np(re.to_new(_dev(torch, S)))
    assert Rn[rank[5]] == R[5]
    for transposed in (False, True):
        a = re.T if transposed else re
        ks, kd = nm.induced_edges(rank[src], rank[dst], n, Rn, Sn, transposed)
        got = _grads(torch, qgtc, a, X, dY, p, q, r, c, mode, needs, **_kw(torch, qgtc, Rn, Sn, n))
        for k, (g, mdl) in enumerate(zip(got, _grad_models(ks, kd, n, X, dY, p, q, r, c, mode, transposed))):
            if g is not None:
                assert_floats_identical(g, mdl, f"reordered {mode} output {k} transposed={transposed}")
    assert not qgtc.tiledAggregate(adj, _dev(torch, X), **kw).requires_grad


# ---- 6. the bitmap and the degrees --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 31, 32, 33, 127, 128, 129, 4097])
def test_node_bitmap(qgtc, n):
    import torch

    rng = np.random.default_rng(n)
    for flags in (rng.random(n) < 0.5, np.ones(n, bool), np.zeros(n, bool), np.arange(n) == n - 1):
        want = nm.bitmap(flags).view(np.int32)
        got = node_bitmap(_dev(torch, flags), n)
        assert got.dtype == torch.int32 and got.is_cuda and got.shape == (nm.bitmap_words(n),)
        np.testing.assert_array_equal(_np(got), want)
        ids = np.flatnonzero(flags).astype(np.int64)
        ids = rng.permutation(np.concatenate([ids, ids[::2], ids[:3]]))      # any order, duplicates
        np.testing.assert_array_equal(_np(node_bitmap(_dev(torch, ids), n)), want)
        assert torch.equal(node_bitmap(_dev(torch, flags), n), got)
    with pytest.raises(ValueError, match="outside"):
        node_bitmap(torch.tensor([0, n], device="cuda"), n)
    with pytest.raises(ValueError, match="outside"):
        node_bitmap(torch.tensor([-1], device="cuda"), n)


def _bitmap_live(env):
    torch = env.torch
    n = 1000
    rng = np.random.default_rng(77)
    src, dst = random_edges(rng, n, 6 * n + 5)
    adj = warm_adjacency(env, src, dst, n)
    flags = [rng.random(n) < 0.5 for _ in range(4)]
    buf = empty(env, (n,), torch.bool)

    def run():
        bm = node_bitmap(buf, n)
        return [bm, adj.mean_scale(row_mask=bm, nbr_mask=bm), adj.T.sym_scale(row_mask=bm, nbr_mask=bm)]

    def want(f):
        ks, kd = nm.induced_edges(src, dst, n, f, f, False)
        return [nm.bitmap(f).view(np.int32), mean_scale(neighbour_lists(ks, kd, n, False)[2]), inv_sqrt_degree(neighbour_lists(ks, kd, n, True)[2])]

    return Live(torch, [buf], [[f] for f in flags], [want(f) for f in flags], run=run, keep=adj)


def test_node_bitmap_and_masked_scales_follow_the_current_stream(qgtc, oracle):
    """tiled.node_bitmap (from flags) and the masked mean_scale / sym_scale reach their C entries through ctypes with the handle of
    torch's current stream: behind a timed head start on three fresh side streams they see the flags copied in on that stream
    (``ordering_probe`` of tests/stream_cases.py), and a captured graph replays them on new flags (``capture_and_replay``)."""
    import torch

    live = _bitmap_live(env_of(qgtc, oracle, torch))
    ordering_probe(torch, qgtc, live, "node bitmap and masked scales")
    capture_and_replay(torch, qgtc, live, "node bitmap and masked scales")


def test_masked_degrees_and_scales(qgtc):
    import torch

    n = 1000
    rng = np.random.default_rng(13)
    src, dst = random_edges(rng, n, 6 * n + 5)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    full = [t.clone() for t in (adj.degrees(), adj.T.degrees(), adj.mean_scale(), adj.sym_scale())]
    for kind in KINDS:
        R, S = _pair(rng, n, kind)
        kw = _kw(torch, qgtc, R, S, n)
        for transposed in (False, True):
            a = adj.T if transposed else adj
            ks, kd = nm.induced_edges(src, dst, n, R, S, transposed)
            kadj = qgtc.pack_edges_tiled(_dev(torch, ks), _dev(torch, kd), n)
            ka = kadj.T if transposed else kadj
            _, _, deg = neighbour_lists(ks, kd, n, transposed)
            d, ms, ss = a.degrees(**kw), a.mean_scale(**kw), a.sym_scale(**kw)
            assert d.dtype == torch.int32 and torch.equal(d, ka.degrees())
            np.testing.assert_array_equal(_np(d), deg)
            assert _same(torch, ms, ka.mean_scale()) and _same(torch, ss, ka.sym_scale())
            assert_floats_identical(_np(ms), mean_scale(deg), "mean scale")
            assert_floats_identical(_np(ss), inv_sqrt_degree(deg), "sym scale")
    # uncached: the unmasked methods give what they gave
    for t, u in zip(full, (adj.degrees(), adj.T.degrees(), adj.mean_scale(), adj.sym_scale())):
        assert torch.equal(t, u)


# ---- 7. the layers ------------------------------------------------------------------------------------------------------------------------------
def _induced(torch, qgtc, src, dst, n, nodes):
    ks, kd = nm.induced_edges(src, dst, n, nodes, nodes, False)
    return qgtc.pack_edges_tiled(_dev(torch, ks), _dev(torch, kd), n)


@pytest.mark.parametrize("norm,aggr", [(None, "sum"), ("mean", "sum"), ("sym", "sum"), (None, "max"), (None, "min")])
def test_gcnconv_on_the_induced_subgraph(qgtc, norm, aggr):
    import torch

    from qgtc_ppopp22_amd import conv

    n, F_in, H, C = 333, 12, 20, 7
    rng = np.random.default_rng(21)
    src, dst = random_edges(rng, n, 6 * n + 5)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    X = _dev(torch, rng.standard_normal((n, F_in)).astype(np.float32))
    nodes = rng.random(n) < 0.5
    torch.manual_seed(0)
    layer = conv.GCNConv(F_in, H, C, norm=norm, aggr=aggr).cuda()
    kadj = _induced(torch, qgtc, src, dst, n, nodes)
    dn = _dev(torch, nodes)
    for a, ka in ((adj, kadj), (adj.T, kadj.T)):
        got, want = layer(a, X, nodes=dn), layer(ka, X)
        assert _same(torch, got, want)
        assert (got[~dn].view(torch.int32) == 0).all()          # rows outside the nodes: +0
        assert not _same(torch, got, layer(a, X))
        layer.zero_grad()
        got.square().mean().backward()
        grads = [w.grad.clone() for w in layer.parameters()]
        layer.zero_grad()
        layer(ka, X).square().mean().backward()
        assert all(_same(torch, g, w.grad) for g, w in zip(grads, layer.parameters()))
    # a reordered adjacency: `nodes` stays in X's numbering and the layer moves it; the re-packed induced adjacency in the same numbering
    re = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n, reorder=True)
    rank = re.rank.cpu().numpy()
    ks, kd = nm.induced_edges(src, dst, n, nodes, nodes, False)
    raw = qgtc.pack_edges_tiled(_dev(torch, rank[ks]), _dev(torch, rank[kd]), n)
    kre = qgtc.TiledAdjacency(n, raw.row_ptr, raw.kquad, raw.tiles, re.perm, re.rank)
    got = layer(re, X, nodes=dn)
    assert _same(torch, got, layer(kre, X)) and (got[~dn].view(torch.int32) == 0).all()


@pytest.mark.parametrize("heads", [1, 3])
def test_gatconv_on_the_induced_subgraph(qgtc, heads):
    import torch

    from qgtc_ppopp22_amd import conv

    n, F_in, C = 333, 12, 9
    rng = np.random.default_rng(22)
    src, dst = random_edges(rng, n, 6 * n + 5)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    X = _dev(torch, rng.standard_normal((n, F_in)).astype(np.float32))
    nodes = rng.random(n) < 0.5
    dn = _dev(torch, nodes)
    torch.manual_seed(0)
    layer = conv.GATConv(F_in, C, heads=heads).cuda()
    kadj = _induced(torch, qgtc, src, dst, n, nodes)
    for a, ka in ((adj, kadj), (adj.T, kadj.T)):
        got = layer(a, X, nodes=dn)
        assert _same(torch, got, layer(ka, X))
        assert (got[~dn].view(torch.int32) == 0).all()
        assert not _same(torch, got, layer(a, X))
        layer.zero_grad()
        got.square().mean().backward()
        grads = [w.grad.clone() for w in layer.parameters()]
        layer.zero_grad()
        layer(ka, X).square().mean().backward()
        assert all(_same(torch, g, w.grad) for g, w in zip(grads, layer.parameters()))


def test_eight_sgd_steps_on_cluster_batches(qgtc):
    """Cluster-GCN on the whole-graph adjacency: eight SGD steps, each on the induced subgraph of another eighth of the nodes, lower the
    loss on the whole graph's labelled rows, and two runs end with identical weight bits."""
    import torch

    from qgtc_ppopp22_amd import conv
    from tiled_sym_model import add_self_loops

    n, F_in, H, C = 1000, 16, 32, 4
    rng = np.random.default_rng(23)
    src, dst = random_edges(rng, n, 6 * n + 5)
    src, dst = add_self_loops(np.concatenate([src, dst]), np.concatenate([dst, src]), n)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    X = _dev(torch, rng.standard_normal((n, F_in)).astype(np.float32))
    W = rng.standard_normal((F_in, C)).astype(np.float32)
    y = _dev(torch, (_np(X) @ W).argmax(axis=1))
    batches = [_dev(torch, (np.arange(n) // 125) == k) for k in range(8)]

    def run():
        torch.manual_seed(0)
        layer = conv.GCNConv(F_in, H, C, norm="sym").cuda()
        with torch.no_grad():
            layer.W_in.mul_(0.1)
            layer.W_out.mul_(0.1)
        opt = torch.optim.SGD(layer.parameters(), lr=0.05)

        def loss_on(nodes):
            return torch.nn.functional.cross_entropy(layer(adj, X, nodes=nodes)[nodes], y[nodes])

        before = float(sum(loss_on(b).detach() for b in batches))
        for b in batches:
            opt.zero_grad()
            loss_on(b).backward()
            opt.step()
        after = float(sum(loss_on(b).detach() for b in batches))
        return before, after, [w.detach().clone() for w in layer.parameters()]

    before, after, w1 = run()
    assert np.isfinite(before) and after < before, (before, after)
    _, _, w2 = run()
    assert all(_same(torch, a, b) for a, b in zip(w1, w2))
