"""All heads of the attention path in one launch (include/qgtc_attn_heads.h; QGTC.tiledMMFloat / tiledAggregate with ``attn=(p, q)`` of
shape [n, H], conv.GATConv) on the device. The contract is that every head is bit for bit what the single-head call gives on the head's
contiguous slice - plain, under ``edge_drop`` and under node masks -, so every comparison here is bit for bit: against the loop over
heads of the existing single-head calls and against tests/tiled_attn_heads_model.py (against NumPy a NaN equals a NaN). Nothing is
sampled and no tolerance is used."""
import ctypes
import functools

import numpy as np
import pytest

import tiled_attn_heads_model as hm
import tiled_drop_model as dm
from test_tiled_float_gpu import CANARY, NAN_WORD, NO_EDGES, assert_floats_identical
from tiled_attn_model import lrelu_f32
from tiled_float_model import neighbour_lists
from tiled_model import random_edges

pytestmark = pytest.mark.gpu

NS = (97, 333)                                   # n % 32 and n % 128 are nonzero; 333 has three k-quads
SHAPES = [(H, d, n) for H, d in hm.HEAD_SHAPES for n in NS] + [(H, d, 97) for H, d in hm.MORE_SHAPES]
DROP = (0.6, 5)


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    return torch


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _same(a, b):
    import torch

    return a.shape == b.shape and torch.equal(a.detach().contiguous().view(torch.int32), b.detach().contiguous().view(torch.int32))


class Graph:
    """The adjacency and its edge list in the adjacency's numbering (`s`, `d`), which the model works on."""

    def __init__(self, n, reorder, edges=None):
        _torch()
        import QGTC

        src, dst = edges if edges is not None else random_edges(np.random.default_rng(17 * n), n, 6 * n + 5)
        self.n = n
        self.adj = QGTC.pack_edges_tiled(_dev(src), _dev(dst), n, reorder=reorder)
        rank = self.adj.rank.cpu().numpy() if reorder else np.arange(n)
        self.s, self.d = rank[src], rank[dst]


@functools.lru_cache(maxsize=None)
def graph(n, reorder=False):
    return Graph(n, reorder)


def _inputs(rng, n, H, d, spread=1.0):
    X, dY = rng.standard_normal((n, H * d)).astype(np.float32), rng.standard_normal((n, H * d)).astype(np.float32)
    p, q = (rng.uniform(-1, 1, (n, H)) * spread).astype(np.float32), (rng.uniform(-1, 1, (n, H)) * spread).astype(np.float32)
    return X, dY, p, q


def _one_call(a, X, p, q, dY, slope, **kw):
    """(Y, m, inv, dX, dp, dq) as device tensors from ONE call for all heads: tiledAggregate under autograd, tiledMMFloat for the
    statistics. X [n, H d], p and q [n, H]."""
    import QGTC

    Xg, pg, qg = (_dev(t).requires_grad_(True) for t in (X, p, q))
    Y = QGTC.tiledAggregate(a, Xg, attn=(pg, qg), negative_slope=slope, **kw)
    assert Y.requires_grad and Y.shape == X.shape and Y.is_contiguous()
    Y.backward(_dev(dY))
    out, m, inv = QGTC.tiledMMFloat(a, Xg.detach(), attn=(pg.detach(), qg.detach()), negative_slope=slope, return_stats=True, **kw)
    assert m.shape == inv.shape == p.shape and m.is_contiguous() and inv.is_contiguous() and _same(out, Y)
    assert _same(QGTC.tiledMMFloat(a, Xg.detach(), attn=(pg.detach(), qg.detach()), negative_slope=slope, **kw), Y)
    assert pg.grad.shape == p.shape and qg.grad.shape == q.shape
    return Y.detach(), m, inv, Xg.grad, pg.grad, qg.grad


def _the_loop(a, X, p, q, dY, slope, **kw):
    """The same six from the loop over heads of single-head calls on contiguous slices, joined."""
    import torch

    H, d = p.shape[1], X.shape[1] // p.shape[1]
    parts = [_one_head(a, X[:, h * d:(h + 1) * d], p[:, h], q[:, h], dY[:, h * d:(h + 1) * d], slope, **kw) for h in range(H)]
    return tuple(torch.cat([pt[i] for pt in parts], dim=1) if i in (0, 3) else torch.stack([pt[i] for pt in parts], dim=1) for i in range(6))


def _one_head(a, X, p, q, dY, slope, **kw):
    import QGTC

    Xg, pg, qg = (_dev(t).requires_grad_(True) for t in (X, p, q))
    Y = QGTC.tiledAggregate(a, Xg, attn=(pg, qg), negative_slope=slope, **kw)
    Y.backward(_dev(dY))
    _, m, inv = QGTC.tiledMMFloat(a, Xg.detach(), attn=(pg.detach(), qg.detach()), negative_slope=slope, return_stats=True, **kw)
    assert m.shape == (a.n,)
    return Y.detach(), m, inv, Xg.grad, pg.grad, qg.grad


def _model(s, d, n, X, p, q, dY, slope, transposed):
    Y, m, inv = hm.attention_heads_f32(s, d, n, X, p, q, slope, transposed)
    dX, dp, dq, _ = hm.attention_grads_heads_f32(s, d, n, X, p, q, dY, Y, m, inv, slope, transposed)
    return Y, m, inv, dX, dp, dq


NAMES = ("Y", "m", "inv", "dX", "dp", "dq")


def _compare(got, loop, want, what, finite=True):
    for name, g, l, w in zip(NAMES, got, loop, want):
        assert _same(g, l), f"{what} {name}: the loop over heads"
        assert_floats_identical(_np(g), w, f"{what} {name}: the model")
        if finite:
            assert np.isfinite(w).all(), f"{what} {name}"


# ---- 1. shapes ------------------------------------------------------------------------------------------------------------------------------
def test_the_shapes_reach_every_path():
    """Against the model's copy of the launchers' switches: both product tables with more than one chunk, lanes whose columns straddle
    heads and lanes whose columns share one, both mappings of DOT and every register class of the score gradient, the one that reads
    its rows again included."""
    shapes = {(H, d) for H, d, _ in SHAPES}
    assert set(hm.HEAD_SHAPES) <= shapes and all((H, d, n) in SHAPES for H, d in hm.HEAD_SHAPES for n in NS)
    for transposed in (False, True):
        assert {hm.product_variant(H, d, transposed) for H, d in shapes} == set(hm.PRODUCT_VARIANTS)
        assert max(hm.product_chunks(H, d, transposed) for H, d in shapes) >= 2
        assert {hm.lanes_straddle_heads(H, d, transposed) for H, d in hm.HEAD_SHAPES} == {False, True}
    assert {hm.grad_variant(H, d)[0] for H, d in shapes} == set(hm.GRAD_VARIANTS)
    assert {hm.grad_variant(H, d)[0][0] for H, d in hm.HEAD_SHAPES} == {"narrow", "wide"}
    assert max(hm.grad_variant(H, d)[1] for H, d in shapes if d <= 64) >= 2
    assert all(n % 32 and n % 128 for n in NS)


@pytest.mark.parametrize("reorder", [False, True], ids=["plain", "reordered"])
@pytest.mark.parametrize("transposed", [False, True], ids=["adj", "adjT"])
@pytest.mark.parametrize("H,d,n", SHAPES, ids=[f"H{H}-d{d}-n{n}" for H, d, n in SHAPES])
def test_every_shape_equals_the_loop_over_heads_and_the_model(H, d, n, transposed, reorder):
    _torch()
    from qgtc_ppopp22_amd import tiled

    g = graph(n, reorder)
    a = g.adj.T if transposed else g.adj
    rng = np.random.default_rng([n, H, d])
    X, dY, p, q = _inputs(rng, n, H, d)
    what = f"H={H} d={d} n={n} product={hm.product_variant(H, d, transposed)} gradient={hm.grad_variant(H, d)}"
    _compare(_one_call(a, X, p, q, dY, 0.2), _the_loop(a, X, p, q, dY, 0.2), _model(g.s, g.d, n, X, p, q, dY, 0.2, transposed), what)
    # the shift: the existing max launch on q as an [n, H] matrix is the single-head max launch per column, and the model's
    Q = _dev(q)
    M = tiled._call(a, "_tiled_mm_f32", Q, reduce="max", return_arg=False)[0]
    assert M.shape == (n, H)
    for h in range(H):
        one = tiled._call(a, "_tiled_mm_f32", Q[:, h].contiguous().unsqueeze(1), reduce="max", return_arg=False)[0]
        assert _same(M[:, h], one.reshape(n)), f"{what}: the shift of head {h}"
    assert_floats_identical(_np(M), hm.max_heads_f32(g.s, g.d, n, q, transposed), f"{what}: the shift")
    # the row dot entry
    D = tiled._att_heads_rowdot(_dev(dY), _dev(X), H)
    assert_floats_identical(_np(D), hm.rowdot_heads_f32(dY, X, H), f"{what}: the row dot")


# ---- 2. masks -------------------------------------------------------------------------------------------------------------------------------
def _kept_on_the_host(s, d, n, rate, seed):
    """the set cells the mask keeps, decided by qgtc_edge_kept on the host"""
    from qgtc_ppopp22_amd import cabi
    from tiled_model import set_cells

    kept_fn, T = cabi.load().qgtc_edge_kept, dm.threshold(rate)
    cells = set_cells(s, d, n)
    keep = np.array([kept_fn(int(c // n), int(c % n), seed, T) == 1 for c in cells], dtype=bool)
    return cells[keep] // n, cells[keep] % n


@pytest.mark.parametrize("transposed", [False, True], ids=["adj", "adjT"])
@pytest.mark.parametrize("H,d", [(3, 5), (8, 8)])
def test_under_edge_dropout(H, d, transposed):
    _torch()
    n = 333
    g = graph(n)
    a = g.adj.T if transposed else g.adj
    ks, kd = _kept_on_the_host(g.s, g.d, n, *DROP)
    mk, md = dm.kept_edges(g.s, g.d, n, dm.threshold(DROP[0]), DROP[1])
    assert np.array_equal(ks, mk) and np.array_equal(kd, md), "qgtc_edge_kept and the model agree"
    for t in (False, True):   # the seed is fit on both views: a row loses every neighbour, another keeps one
        before, after = neighbour_lists(g.s, g.d, n, t)[2], neighbour_lists(ks, kd, n, t)[2]
        assert ((before > 0) & (after == 0)).any() and (after > 0).any() and (after < before).any()
    rng = np.random.default_rng([n, H, d, 2])
    X, dY, p, q = _inputs(rng, n, H, d)
    kw = dict(edge_drop=DROP)
    _compare(_one_call(a, X, p, q, dY, 0.2, **kw), _the_loop(a, X, p, q, dY, 0.2, **kw), _model(ks, kd, n, X, p, q, dY, 0.2, transposed),
             f"edge_drop H={H} d={d}")


@pytest.mark.parametrize("transposed", [False, True], ids=["adj", "adjT"])
@pytest.mark.parametrize("H,d", [(3, 5), (8, 8)])
def test_under_node_masks(H, d, transposed):
    _torch()
    from qgtc_ppopp22_amd import tiled

    n = 333
    g = graph(n)
    a = g.adj.T if transposed else g.adj
    rng = np.random.default_rng([n, H, d, 3])
    inside = rng.random(n) < 1 / 3
    bm = tiled.node_bitmap(_dev(inside), n)
    keep = inside[g.s] & inside[g.d]
    X, dY, p, q = _inputs(rng, n, H, d)
    X[~inside] = np.nan   # a node outside the masks is never loaded
    kw = dict(row_mask=bm, nbr_mask=bm)
    got, loop = _one_call(a, X, p, q, dY, 0.2, **kw), _the_loop(a, X, p, q, dY, 0.2, **kw)
    Xin = np.where(inside[:, None], X, np.float32(0))
    want = _model(g.s[keep], g.d[keep], n, Xin, p, q, dY, 0.2, transposed)
    _compare(got, loop, want, f"node masks H={H} d={d}")
    assert (_np(got[0])[~inside].view(np.uint32) == 0).all() and (_np(got[3])[~inside].view(np.uint32) == 0).all()


# ---- 3. a hub -------------------------------------------------------------------------------------------------------------------------------
def test_a_long_row_and_a_long_column():
    """Hub h has 300 out-edges and 300 in-edges at n = 600: its row queues more than 32 neighbours (full queues are flushed), its
    k-quad's list has more than 8 tiles (several rounds of the column view)."""
    _torch()
    n, h, H, d = 600, 301, 4, 16
    rng = np.random.default_rng(4)
    others = rng.permutation(np.delete(np.arange(n, dtype=np.int64), h))[:300]
    extra = random_edges(rng, n, 2 * n)
    keep = (extra[0] != h) & (extra[1] != h)
    src = np.concatenate([np.full(300, h, np.int64), others, extra[0][keep]])
    dst = np.concatenate([others, np.full(300, h, np.int64), extra[1][keep]])
    g = Graph(n, False, (src, dst))
    t = g.adj.T
    assert int(g.adj.degrees()[h]) == 300 and int(t.degrees()[h]) == 300
    assert int((t.col_ptr[h // 128 + 1] - t.col_ptr[h // 128]).item()) > 8
    X, dY, p, q = _inputs(rng, n, H, d, spread=3.0)
    for transposed in (False, True):
        a = t if transposed else g.adj
        _compare(_one_call(a, X, p, q, dY, 0.2), _the_loop(a, X, p, q, dY, 0.2), _model(src, dst, n, X, p, q, dY, 0.2, transposed),
                 f"hub transposed={transposed}")


def _masked_scores(rng, s, d, n, q, transposed):
    """q with about 40 % of the nodes at -inf, such that every row of the view keeps an unmasked neighbour"""
    o, k, deg = neighbour_lists(s, d, n, transposed)
    masked = rng.random(n) < 0.4
    alive = np.bincount(o[~masked[k]], minlength=n) > 0
    for r in np.flatnonzero((deg > 0) & ~alive):   # unmasking only ever keeps rows alive
        masked[k[o == r][-1]] = False
    assert (np.bincount(o[~masked[k]], minlength=n) > 0)[deg > 0].all()
    return np.where(masked, -np.inf, q).astype(np.float32)


# ---- 4. special scores, per head ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slope", [0.0, 0.2, 1.0])
def test_special_scores_stay_with_their_head(slope):
    """One call: head 0 has scores up to +-200 (many weights are exactly 0), head 1 has neighbours masked by -inf (slope > 0: at slope
    0 the logit of a masked neighbour is 0 . inf) which the other heads keep, head 2 has scores on a grid of eighths, so e is exactly 0
    on many edges, where the slope applies in the gradient; head 3 is plain."""
    _torch()
    n, H, d = 333, 4, 6
    g = graph(n)
    rng = np.random.default_rng([n, 44])
    X, dY, p, q = _inputs(rng, n, H, d)
    p[:, 0], q[:, 0] = p[:, 0] * 200, q[:, 0] * 200
    p[:, 2], q[:, 2] = rng.integers(-8, 9, n) / 8, rng.integers(-8, 9, n) / 8
    for transposed in (False, True):
        a = g.adj.T if transposed else g.adj
        qq = q.copy()
        if slope > 0:
            qq[:, 1] = _masked_scores(rng, g.s, g.d, n, q[:, 1], transposed)
            assert np.isinf(qq[:, 1]).sum() > n // 5 and np.isfinite(np.delete(qq, 1, axis=1)).all()
        o, k, _ = neighbour_lists(g.s, g.d, n, transposed)
        want = _model(g.s, g.d, n, X, p, qq, dY, slope, transposed)
        with np.errstate(all="ignore"):
            assert ((lrelu_f32(p[o, 0] + qq[k, 0], slope) - want[1][o, 0]) < -87).sum() > n
        assert ((p[o, 2] + qq[k, 2]) == 0).sum() > 20
        got = _one_call(a, X, p, qq, dY, slope)
        _compare(got, _the_loop(a, X, p, qq, dY, slope), want, f"special slope={slope} transposed={transposed}")
        if slope > 0:
            assert (_np(got[5])[np.isinf(qq[:, 1]), 1] == 0).all()      # a masked neighbour takes part in nothing, in its head
            assert (_np(got[5])[np.isinf(qq[:, 1]), 3] != 0).any()      # and in the others as ever


# ---- 5. edge cases ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,H,d,loop", [(1, 2, 1, False), (1, 3, 5, True), (300, 4, 6, False), (97, 2, 150, False)])
def test_an_empty_adjacency_and_one_node(n, H, d, loop):
    _torch()
    rng = np.random.default_rng(n + H)
    src, dst = (np.zeros(1, np.int64), np.zeros(1, np.int64)) if loop else NO_EDGES
    g = Graph(n, False, (src, dst))
    assert g.adj.n_tiles == (1 if loop else 0)
    X, dY, p, q = _inputs(rng, n, H, d)
    for transposed in (False, True):
        a = g.adj.T if transposed else g.adj
        got = _one_call(a, X, p, q, dY, 0.2)
        _compare(got, _the_loop(a, X, p, q, dY, 0.2), _model(src, dst, n, X, p, q, dY, 0.2, transposed), f"n={n} loop={loop}")
        if loop:
            assert_floats_identical(_np(got[0]), X, "one self loop: the softmax of one logit is 1")
        else:
            assert all((_np(t).view(np.uint32) == 0).all() for t in (got[0], got[2], got[3], got[4], got[5]))
            assert_floats_identical(_np(got[1]), lrelu_f32(p, 0.2), "m of a row without neighbours is L(p)")


def test_a_gradient_not_required_is_not_launched(monkeypatch):
    _torch()
    import QGTC
    from qgtc_ppopp22_amd import tiled

    n, H, d = 97, 3, 5
    g = graph(n)
    rng = np.random.default_rng(6)
    X, dY, p, q = _inputs(rng, n, H, d)
    calls = []
    for name in ("_att_heads_product", "_att_heads_grad", "_att_heads_rowdot", "_att"):
        fn = getattr(tiled, name)
        monkeypatch.setattr(tiled, name, lambda *a, _fn=fn, _name=name, **k: (calls.append((_name, a[-5] if _name == "_att_heads_grad" else None)), _fn(*a, **k))[1])
    want = {0b001: ["_att_heads_product"], 0b010: ["_att_heads_rowdot", ("_att_heads_grad", False)],
            0b100: ["_att_heads_rowdot", ("_att_heads_grad", True)],
            0b111: ["_att_heads_product", "_att_heads_rowdot", ("_att_heads_grad", False), ("_att_heads_grad", True)]}
    for a in (g.adj, g.adj.T):
        full = _one_call(a, X, p, q, dY, 0.2)[3:]
        for mask in range(1, 8):
            ts = [_dev(t).requires_grad_(bool(mask >> i & 1)) for i, t in enumerate((X, p, q))]
            Y = QGTC.tiledAggregate(a, ts[0], attn=(ts[1], ts[2]))
            calls.clear()
            Y.backward(_dev(dY))
            for i, t in enumerate(ts):
                assert (t.grad is None) == (not mask >> i & 1)
                if t.grad is not None:
                    assert _same(t.grad, full[i]), f"subset {mask:03b} gradient {i}"
            if mask in want:
                assert [c[0] if c[1] is None else c for c in calls] == want[mask], f"subset {mask:03b}"
            assert len(calls) <= 4 and all(c[0] != "_att" for c in calls)
        ts = [_dev(t) for t in (X, p, q)]
        calls.clear()
        assert not QGTC.tiledAggregate(a, ts[0], attn=(ts[1], ts[2])).requires_grad
        assert [c[0] for c in calls] == ["_att_heads_product"], "the forward: the max launch and one product launch"
    # a non-contiguous dY is made contiguous by the backward; and there is no second derivative
    import torch

    Xg = _dev(X).requires_grad_(True)
    wide = _dev(np.repeat(dY, 2, axis=1))
    QGTC.tiledAggregate(g.adj, Xg, attn=(_dev(p), _dev(q))).backward(wide[:, ::2])
    assert _same(Xg.grad, _one_call(g.adj, X, p, q, dY, 0.2)[3]), "strided dY"
    Xg = _dev(X).requires_grad_(True)
    gx, = torch.autograd.grad(QGTC.tiledAggregate(g.adj, Xg, attn=(_dev(p), _dev(q))), Xg, _dev(dY), create_graph=True)
    with pytest.raises(RuntimeError):
        gx.sum().backward()


def _view_ptrs(a):
    t = (a.col_ptr, a.col_tile, a.col_rb, a.tiles) if a.transposed else (a.row_ptr, a.kquad, a.tiles)
    return tuple(x.data_ptr() for x in t) + (a.n_tiles, a.n)


def _fresh(elems):
    import torch

    return torch.full((elems + CANARY,), float("nan"), dtype=torch.float32, device="cuda")


def _taken(buf, elems):
    a = buf.cpu().numpy()
    assert (a[elems:].view(np.uint32) == NAN_WORD).all(), "canaries"
    return a[:elems]


@pytest.mark.parametrize("mask", ["", "_drop", "_nodes"])
@pytest.mark.parametrize("transposed", [False, True], ids=["adj", "adjT"])
@pytest.mark.parametrize("H,d", [(1, 5), (1, 70), (3, 5), (2, 65)])
def test_the_c_entries_with_canaries_and_one_head_against_the_twin(H, d, transposed, mask):
    """Every entry on raw device pointers with canaries behind every output, against the model; with heads = 1 also against its
    single-head twin, bit for bit."""
    torch = _torch()
    import QGTC
    from qgtc_ppopp22_amd import cabi, tiled

    L = cabi.load()
    n, N = 97, H * d
    g = graph(n)
    a, other = (g.adj.T, g.adj) if transposed else (g.adj, g.adj.T)
    rng = np.random.default_rng([n, H, d, 9])
    X, dY, p, q = _inputs(rng, n, H, d)
    inside = rng.random(n) < 0.5
    bm = tiled.node_bitmap(_dev(inside), n)
    tail = {"": (), "_drop": (dm.threshold(DROP[0]), DROP[1]), "_nodes": (bm.data_ptr(), bm.data_ptr(), bm.numel())}[mask]
    kw = {"": {}, "_drop": dict(edge_drop=DROP), "_nodes": dict(row_mask=bm, nbr_mask=bm)}[mask]
    s, e = {"": (g.s, g.d), "_drop": dm.kept_edges(g.s, g.d, n, dm.threshold(DROP[0]), DROP[1]),
            "_nodes": (g.s[inside[g.s] & inside[g.d]], g.d[inside[g.s] & inside[g.d]])}[mask]
    Y, m, inv, gX, gp, gq = _model(s, e, n, X, p, q, dY, 0.2, transposed)
    D = hm.rowdot_heads_f32(dY, Y, H)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    sfx = ("_t" if transposed else "") + mask
    dX_, ddY, dp_, dq_, dm_, di_, dD_, dY_ = (_dev(t) for t in (X, dY, p, q, m, inv, D, Y))
    M = QGTC.tiledMMFloat(a, dq_, reduce="max", **kw)
    vp, vo = _view_ptrs(a), _view_ptrs(other)
    osfx = ("" if transposed else "_t") + mask
    otail = (tail[1], tail[0], tail[2]) if mask == "_nodes" else tail

    def run(heads, name, *args):
        rc = getattr(L, name)(*args)
        assert rc == 0, (name, L.qgtc_strerror(rc).decode())

    def forward(fn_heads):
        out, mo, io = _fresh(n * N), _fresh(n * H), _fresh(n * H)
        args = (*vp, dX_.data_ptr(), n * N, N, dp_.data_ptr(), dq_.data_ptr(), 0.2, 0, M.data_ptr(), mo.data_ptr(), io.data_ptr(),
                out.data_ptr(), n * N)
        run(H, "qgtc_tiledatt" + ("_heads" if fn_heads else "") + "_f32" + sfx, *args, *((H,) if fn_heads else ()), *tail, st)
        return _taken(out, n * N).reshape(n, N), _taken(mo, n * H).reshape(n, H), _taken(io, n * H).reshape(n, H)

    def backward(fn_heads):   # the gradient for X runs on the other view
        out = _fresh(n * N)
        args = (*vo, ddY.data_ptr(), n * N, N, dq_.data_ptr(), dp_.data_ptr(), 0.2, 1, dm_.data_ptr(), None, di_.data_ptr(), out.data_ptr(),
                n * N)
        run(H, "qgtc_tiledatt" + ("_heads" if fn_heads else "") + "_f32" + osfx, *args, *((H,) if fn_heads else ()), *otail, st)
        return _taken(out, n * N).reshape(n, N)

    def grad(fn_heads, nbr_owns):
        out = _fresh(n * H)
        view, A, B, own, nbr, sf, tl = ((vo, dX_, ddY, dq_, dp_, osfx, otail) if nbr_owns else (vp, ddY, dX_, dp_, dq_, sfx, tail))
        args = (*view, A.data_ptr(), B.data_ptr(), n * N, N, own.data_ptr(), nbr.data_ptr(), 0.2, int(nbr_owns), dm_.data_ptr(), di_.data_ptr(),
                dD_.data_ptr(), out.data_ptr(), n * H)
        run(H, "qgtc_tiledatt_grad" + ("_heads" if fn_heads else "") + "_f32" + sf, *args, *((H,) if fn_heads else ()), *tl, st)
        return _taken(out, n * H).reshape(n, H)

    def rowdot(fn_heads):
        out = _fresh(n * H)
        run(H, "qgtc_rowdot" + ("_heads" if fn_heads else "") + "_f32", ddY.data_ptr(), dY_.data_ptr(), n * N, n, N, out.data_ptr(), n * H,
            *((H,) if fn_heads else ()), st)
        return _taken(out, n * H).reshape(n, H)

    got = (*forward(True), backward(True), grad(True, False), grad(True, True))
    for name, gt, w in zip(NAMES, got, (Y, m, inv, gX, gp, gq)):
        assert_floats_identical(gt, w, f"C {name} H={H} d={d}{sfx}")
    assert_floats_identical(rowdot(True), D, "C row dot")
    if H == 1:
        twin = (*forward(False), backward(False), grad(False, False), grad(False, True))
        for name, gt, tw in zip(NAMES, got, twin):
            assert (gt.view(np.uint32) == tw.view(np.uint32)).all(), f"heads = 1 against the twin: {name}{sfx}"
        assert (rowdot(True).view(np.uint32) == rowdot(False).view(np.uint32)).all()


def test_refusals():
    torch = _torch()
    import QGTC

    n, H, d = 97, 3, 5
    g = graph(n)
    X = torch.ones(n, H * d, dtype=torch.float32, device="cuda")
    s = torch.ones(n, H, dtype=torch.float32, device="cuda")
    v = torch.ones(n, dtype=torch.float32, device="cuda")
    for a in (g.adj, g.adj.T):
        for fn in (QGTC.tiledMMFloat, QGTC.tiledAggregate):
            assert fn(a, X, attn=(s, s)).shape == (n, H * d)
            with pytest.raises(ValueError, match="3 heads, which do not divide X's 16 columns"):
                fn(a, torch.ones(n, 16, dtype=torch.float32, device="cuda"), attn=(s, s))
            with pytest.raises(ValueError, match="the same shape"):
                fn(a, X, attn=(s, v))
            with pytest.raises(ValueError, match="the same shape"):
                fn(a, X, attn=(s, s[:, :2].contiguous()))
            with pytest.raises(ValueError, match="the same shape"):
                fn(a, X, attn=(s[:-1], s))
            with pytest.raises(TypeError, match="att_out must be float32"):
                fn(a, X, attn=(s.double(), s))
            with pytest.raises(TypeError, match="att_nbr must be a torch.Tensor"):
                fn(a, X, attn=(s, [[1.0] * H] * n))
            with pytest.raises(ValueError, match="att_nbr must be on the adjacency's device"):
                fn(a, X, attn=(s, s.cpu()))
            with pytest.raises(ValueError, match="att_out must be contiguous"):
                fn(a, X, attn=(torch.ones(n, 2 * H, device="cuda")[:, ::2], s))
            # [n, 1] stays refused, in the words it always was
            with pytest.raises(ValueError, match=r"att_out must have shape \[97\]"):
                fn(a, X, attn=(v.unsqueeze(1), v.unsqueeze(1)))
            # what one head refuses, heads refuse in the same words
            with pytest.raises(ValueError, match="row_scale cannot be combined with attn"):
                fn(a, X, row_scale=v, attn=(s, s))
            with pytest.raises(ValueError, match="negative_slope"):
                fn(a, X, attn=(s, s), negative_slope=1.5)
            with pytest.raises(ValueError, match="edge_weight cannot be combined with attn: not built"):
                fn(a, X, attn=(s, s), edge_weight=v)
        with pytest.raises(ValueError, match="return_arg cannot be combined with attn"):
            QGTC.tiledMMFloat(a, X, attn=(s, s), return_arg=True)


# ---- 6. the layer -----------------------------------------------------------------------------------------------------------------------------
def _per_head_layer(layer, A, X, drop=None, mask=None):
    """conv.GATConv.forward as it was before the heads shared a call: a loop over the heads, from public single-head calls"""
    import QGTC
    import torch

    h = torch.mm(A.to_new(X), layer.W)
    outs = []
    for i in range(layer.heads):
        hi = h[:, i * layer.output_dim:(i + 1) * layer.output_dim].contiguous()
        p, q = torch.mv(hi, layer.a_dst[i]), torch.mv(hi, layer.a_src[i])
        outs.append(QGTC.tiledAggregate(A, hi, attn=(p, q), negative_slope=layer.negative_slope, edge_drop=drop, **(mask or {})))
    return A.to_old(torch.cat(outs, dim=1) if layer.concat else torch.stack(outs).mean(dim=0))


@pytest.mark.parametrize("how", ["plain", "edge_drop", "nodes"])
@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("heads", [3, 8])
def test_gatconv_equals_its_per_head_loop(heads, concat, how):
    """Forward and one SGD step: the output and the gradients of W, a_dst and a_src, bit for bit."""
    torch = _torch()
    from qgtc_ppopp22_amd import tiled
    from qgtc_ppopp22_amd.conv import GATConv

    n, fin, dout = 333, 12, 8
    g = graph(n, True)
    rng = np.random.default_rng([heads, int(concat)])
    X = _dev(rng.standard_normal((n, fin)).astype(np.float32))
    dY = _dev(rng.standard_normal((n, heads * dout if concat else dout)).astype(np.float32))
    for A in (g.adj, g.adj.T):
        torch.manual_seed(heads)
        layer = GATConv(fin, dout, heads=heads, concat=concat, edge_drop=0.5 if how == "edge_drop" else 0.0).cuda()
        layer.train()
        kw, ref_kw = {}, {}
        if how == "edge_drop":
            kw, ref_kw = dict(edge_seed=11), dict(drop=(0.5, 11))
        elif how == "nodes":
            inside = _dev(rng.random(n) < 0.5)
            bm = tiled.node_bitmap(A.to_new(inside), n)
            kw, ref_kw = dict(nodes=inside), dict(mask=dict(row_mask=bm, nbr_mask=bm))
        out = layer(A, X, **kw)
        out.backward(dY)
        got = [t.grad.clone() for t in (layer.W, layer.a_dst, layer.a_src)]
        for t in (layer.W, layer.a_dst, layer.a_src):
            t.grad = None
        ref = _per_head_layer(layer, A, X, **ref_kw)
        ref.backward(dY)
        assert _same(out, ref), f"{how}: the output"
        for name, gt, t in zip(("W", "a_dst", "a_src"), got, (layer.W, layer.a_dst, layer.a_src)):
            assert _same(gt, t.grad), f"{how}: the gradient of {name}"
        with torch.no_grad():   # one SGD step lands on the same parameters
            for gt, t in zip(got, (layer.W, layer.a_dst, layer.a_src)):
                assert _same(t - 0.1 * gt, t - 0.1 * t.grad)
