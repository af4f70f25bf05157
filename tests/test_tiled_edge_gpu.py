"""The edge values of the tiled adjacency on the device (tiled.edge_slots / edge_endpoints / edge_values,
QGTC.tiledMMFloat(edge_weight=) on adj and adj.T, tiled.tiledSDDMM, QGTC.tiledAggregate(edge_weight=) and conv.GCNConv(edge_weight=))
against the exact model of tests/tiled_edge_model.py and against the existing kernels. The order of the adds is part of the contract,
so every comparison is bit for bit (against the NumPy model a NaN equals a NaN); nothing is sampled and no tolerance is used.

Graphs: n in {1, 33, 129, 300} (a partial row block, a partial k-quad, 10 row blocks); at n = 300 one node adjacent to every row (its
k-quad's column list exceeds the 8 tiles of a round), one tile with all cells set (a row queue overflows TILED_F32_CAP, val_row reaches
its largest values), a row and a column without edges; n = 300 once more with reorder=True."""
import functools

import numpy as np
import pytest

import tiled_edge_model as em
from tiled_model import random_edges, set_cells

pytestmark = pytest.mark.gpu

NS = (1, 33, 129, 300)
WIDTHS = (1, 16, 17, 33, 64, 65, 129, 257, 300)
GRAPHS = [(n, False) for n in NS] + [(300, True)]


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    return torch


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def assert_floats_identical(got, want, what=""):
    """Bit for bit (so -0.0 is not 0.0), except that any NaN equals any NaN."""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    np.testing.assert_array_equal(gn, wn, err_msg=f"{what}: NaN positions")
    np.testing.assert_array_equal(got.view(np.uint32)[~gn], want.view(np.uint32)[~wn], err_msg=what)


def same_bits(a, b):
    import torch

    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class Graph:
    """One test graph: the edge list as given (`src`, `dst`), the adjacency, and the edge list in the adjacency's numbering (`s`, `d`,
    NumPy) that the model works on."""

    def __init__(self, n, reorder):
        torch = _torch()
        import QGTC

        rng = np.random.default_rng(100 + n)
        src, dst = (np.asarray(a, dtype=np.int64) for a in random_edges(rng, n, max(4, 4 * n)))
        if n == 300:
            every = np.arange(n)
            full_r, full_c = np.meshgrid(np.arange(32, 64), np.arange(128, 256), indexing="ij")
            # the random edges stay out of the hub column and the full tile: a second copy of a cell would unset it
            keep = (dst != 7) & ~((src >= 32) & (src < 64) & (dst >= 128) & (dst < 256))
            src, dst = src[keep], dst[keep]
            src = np.concatenate([src, every, full_r.ravel()])
            dst = np.concatenate([dst, np.full(n, 7), full_c.ravel()])
        if n >= 33:   # row 5 and column 9 without edges
            keep = (src != 5) & (dst != 9)
            src, dst = src[keep], dst[keep]
        self.n, self.src, self.dst = n, src, dst
        self.adj = QGTC.pack_edges_tiled(_dev(src), _dev(dst), n, reorder=reorder)
        if reorder:
            rank = self.adj.rank.cpu().numpy()
            ok = (src >= 0) & (src < n) & (dst >= 0) & (dst < n)
            self.s, self.d = rank[src[ok]], rank[dst[ok]]
        else:
            self.s, self.d = src, dst
        self.row, self.col = em.slot_cells(self.s, self.d, n)
        self.nnz = self.row.size
        self.values = np.random.default_rng(n).normal(size=self.nnz).astype(np.float32)
        self.scale = np.random.default_rng(n + 1).uniform(0.5, 2.0, n).astype(np.float32)

    def X(self, N, special=True):
        X = np.random.default_rng(self.n * 1000 + N).normal(size=(self.n, N)).astype(np.float32)
        if special:
            X[3 % self.n, 0] = np.nan
            X[3 % self.n, N - 1] = np.inf
        return X


@functools.lru_cache(maxsize=None)
def graph(n, reorder=False):
    return Graph(n, reorder)


def test_the_shapes_hit_every_variant():
    assert {em.edge_variant(N, False) for N in WIDTHS} == set(em.EDGE_FORWARD_VARIANTS)
    assert {em.edge_variant(N, True) for N in WIDTHS} == set(em.EDGE_TRANSPOSED_VARIANTS)
    assert {em.sddmm_variant(N) for N in WIDTHS} == set(em.SDDMM_VARIANTS)
    # more than one workgroup along the width on both views
    assert 300 > 256 and 65 > 64
    g = graph(300)
    val_ptr, val_row = em.value_index(g.s, g.d, g.n)
    assert val_row.max() == 31 * 128, "the full tile: val_row reaches its largest value"
    assert (np.bincount(g.row, minlength=g.n) >= 128).any(), "a row queue overflows the cap several times"
    assert np.bincount(g.row, minlength=g.n)[5] == 0 and np.bincount(g.col, minlength=g.n)[9] == 0
    assert np.unique(g.row[g.col >> 7 == 0] >> 5).size > 8, "a column list longer than a round"


@pytest.mark.parametrize("n,reorder", GRAPHS)
def test_slots_and_endpoints(n, reorder):
    torch = _torch()
    from qgtc_ppopp22_amd import tiled

    g = graph(n, reorder)
    adj = g.adj
    val_ptr, val_row, nnz = tiled._value_index(adj)
    mp, mr = em.value_index(g.s, g.d, n)
    assert nnz == g.nnz and np.array_equal(val_ptr.cpu().numpy(), mp) and np.array_equal(val_row.cpu().numpy(), mr)
    row, col = tiled.edge_endpoints(adj)
    assert row.dtype == torch.int32 and np.array_equal(row.cpu().numpy(), g.row) and np.array_equal(col.cpu().numpy(), g.col)
    assert tiled.edge_endpoints(adj.T)[0] is row
    # the slots of the stored cells, named in the edge list's ids
    r64, c64 = row.long(), col.long()
    if reorder:
        r64, c64 = adj.perm[r64], adj.perm[c64]
    assert torch.equal(tiled.edge_slots(adj, r64, c64), torch.arange(nnz, device="cuda"))
    assert torch.equal(tiled.edge_slots(adj.T, r64, c64), torch.arange(nnz, device="cuda"))
    # the raw edge list: the model's answer for every edge, -1 for the cells multiplicity 2 quantised away
    got = tiled.edge_slots(adj, _dev(g.src), _dev(g.dst)).cpu().numpy()
    assert np.array_equal(got, em.edge_slots(g.s, g.d, n, g.s, g.d))
    if n >= 33:
        assert (got == -1).any(), "the edge list holds doubled edges"
    bad_s = torch.tensor([-1, n, 0, 5 % n, 1 << 40], device="cuda")
    bad_d = torch.tensor([0, 0, n, 0, 0], device="cuda")
    want = [-1, -1, -1, -1 if n >= 33 else int(em.edge_slots(g.s, g.d, n, [5 % n], [0])[0]), -1]
    assert tiled.edge_slots(adj, bad_s, bad_d).tolist() == want


@pytest.mark.parametrize("N", WIDTHS)
@pytest.mark.parametrize("n,reorder", GRAPHS)
def test_weighted_forward_equals_the_model(n, reorder, N):
    _torch()
    import QGTC

    g = graph(n, reorder)
    X = g.X(N)
    dX, dv, ds = _dev(X), _dev(g.values), _dev(g.scale)
    for transposed in (False, True):
        a = g.adj.T if transposed else g.adj
        for scale, dscale in ((None, None), (g.scale, ds)):
            got = QGTC.tiledMMFloat(a, dX, dscale, edge_weight=dv).cpu().numpy()
            assert_floats_identical(got, em.weighted_f32(g.s, g.d, n, X, g.values, transposed, scale), f"T={transposed} scaled={scale is not None}")


@pytest.mark.parametrize("N", WIDTHS)
@pytest.mark.parametrize("n,reorder", [(33, False), (300, False), (300, True)])
def test_weighted_forward_equals_the_existing_kernels(n, reorder, N):
    torch = _torch()
    import QGTC
    from qgtc_ppopp22_amd import tiled

    g = graph(n, reorder)
    dX, ds = _dev(g.X(N, special=False)), _dev(g.scale)
    c = _dev(np.random.default_rng(N).normal(size=n).astype(np.float32))
    row, col = tiled.edge_endpoints(g.adj)
    ones = torch.ones(g.nnz, device="cuda")
    for a in (g.adj, g.adj.T):
        for sc in (None, ds):
            assert same_bits(QGTC.tiledMMFloat(a, dX, sc, edge_weight=ones), QGTC.tiledMMFloat(a, dX, sc)), (a.transposed, sc is not None)
    for sc in (None, ds):
        assert same_bits(QGTC.tiledMMFloat(g.adj, dX, sc, edge_weight=c[col.long()]), QGTC.tiledMMFloat(g.adj, dX, sc, src_scale=c))
        assert same_bits(QGTC.tiledMMFloat(g.adj.T, dX, sc, edge_weight=c[row.long()]), QGTC.tiledMMFloat(g.adj.T, dX, sc, src_scale=c))


@pytest.mark.parametrize("N", WIDTHS)
@pytest.mark.parametrize("n,reorder", GRAPHS)
def test_sddmm_equals_the_model(n, reorder, N):
    _torch()
    from qgtc_ppopp22_amd import tiled

    g = graph(n, reorder)
    rng = np.random.default_rng(N + 7)
    A, B = rng.normal(size=(n, N)).astype(np.float32), rng.normal(size=(n, N)).astype(np.float32)
    dA, dB = _dev(A), _dev(B)
    got = tiled.tiledSDDMM(g.adj, dA, dB)
    assert got.shape == (g.nnz,)
    assert_floats_identical(got.cpu().numpy(), em.sddmm_f32(g.s, g.d, n, A, B), "adj")
    assert_floats_identical(got.cpu().numpy(), em.DOT(A[g.row], B[g.col]), "per edge DOT(dY[i], X[j])")
    assert_floats_identical(tiled.tiledSDDMM(g.adj.T, dA, dB).cpu().numpy(), em.sddmm_f32(g.s, g.d, n, A, B, transposed=True), "adj.T")


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("n,reorder", [(33, False), (300, False), (300, True)])
def test_autograd_is_exact_on_small_integers(n, reorder, transposed):
    torch = _torch()
    import QGTC

    g = graph(n, reorder)
    a = g.adj.T if transposed else g.adj
    rng = np.random.default_rng(n + 3)
    N = 17
    # |w| <= 2, |x| <= 3, |dY| <= 3, r in {1, 2}, degree <= 300: every sum stays far below 2^24
    Xn = rng.integers(-3, 4, (n, N)).astype(np.float32)
    vn = rng.integers(-2, 3, g.nnz).astype(np.float32)
    dYn = rng.integers(-3, 4, (n, N)).astype(np.float32)
    rn = rng.integers(1, 3, n).astype(np.float32)
    W = torch.zeros((n, n), dtype=torch.float64)
    for scaled in (False, True):
        r = _dev(rn) if scaled else None
        X, v = _dev(Xn).requires_grad_(True), _dev(vn).requires_grad_(True)
        Y = QGTC.tiledAggregate(a, X, r, edge_weight=v)
        Y.backward(_dev(dYn))
        # the dense float64 route
        X64 = torch.from_numpy(Xn).double().requires_grad_(True)
        v64 = torch.from_numpy(vn).double().requires_grad_(True)
        W64 = W.index_put((torch.from_numpy(g.row), torch.from_numpy(g.col)), v64)
        Y64 = (W64.t() if transposed else W64) @ X64
        if scaled:
            Y64 = torch.from_numpy(rn).double()[:, None] * Y64
        Y64.backward(torch.from_numpy(dYn).double())
        assert float(Y64.abs().max()) < 2 ** 24
        assert torch.equal(Y.detach().cpu().double(), Y64.detach())
        assert torch.equal(X.grad.cpu().double(), X64.grad) and torch.equal(v.grad.cpu().double(), v64.grad)
        # two runs give the same bits
        X2, v2 = _dev(Xn).requires_grad_(True), _dev(vn).requires_grad_(True)
        QGTC.tiledAggregate(a, X2, r, edge_weight=v2).backward(_dev(dYn))
        assert same_bits(X2.grad, X.grad) and same_bits(v2.grad, v.grad)
        # a gradient that is not required is not computed: each alone
        X3, v3 = _dev(Xn), _dev(vn).requires_grad_(True)
        QGTC.tiledAggregate(a, X3, r, edge_weight=v3).backward(_dev(dYn))
        assert X3.grad is None and same_bits(v3.grad, v.grad)
        X4, v4 = _dev(Xn).requires_grad_(True), _dev(vn)
        QGTC.tiledAggregate(a, X4, r, edge_weight=v4).backward(_dev(dYn))
        assert v4.grad is None and same_bits(X4.grad, X.grad)


def test_a_gradient_not_required_is_not_launched(monkeypatch):
    torch = _torch()
    import QGTC
    from qgtc_ppopp22_amd import tiled

    g = graph(33)
    calls = []
    real_sddmm, real_mm = tiled.tiledSDDMM, tiled.tiledMMFloat
    monkeypatch.setattr(tiled, "tiledSDDMM", lambda *a, **k: (calls.append("sddmm"), real_sddmm(*a, **k))[1])
    monkeypatch.setattr(tiled, "tiledMMFloat", lambda *a, **k: (calls.append("mm"), real_mm(*a, **k))[1])
    X, v = _dev(g.X(5, special=False)), _dev(g.values).requires_grad_(True)
    QGTC.tiledAggregate(g.adj, X, edge_weight=v).sum().backward()
    assert calls == ["mm", "sddmm"] and v.grad is not None
    calls.clear()
    X, v = X.clone().requires_grad_(True), _dev(g.values)
    QGTC.tiledAggregate(g.adj, X, edge_weight=v).sum().backward()
    assert calls == ["mm", "mm"] and X.grad is not None
    X5, v5 = X.detach().clone().requires_grad_(True), _dev(g.values).requires_grad_(True)
    gx, = torch.autograd.grad(QGTC.tiledAggregate(g.adj, X5, edge_weight=v5).sum(), X5, create_graph=True)
    with pytest.raises(RuntimeError):   # once_differentiable: no second derivative
        gx.sum().backward()


def test_refusals():
    torch = _torch()
    import QGTC
    from qgtc_ppopp22_amd import tiled

    g = graph(129)
    adj, X, v = g.adj, _dev(g.X(8, special=False)), _dev(g.values)
    bm = tiled.node_bitmap(torch.ones(g.n, dtype=torch.bool, device="cuda"), g.n)
    z = torch.zeros(g.n, device="cuda")
    for fn in (QGTC.tiledMMFloat, QGTC.tiledAggregate):
        for kw in ({"src_scale": _dev(g.scale)}, {"edge_drop": (0.5, 1)}, {"row_mask": bm}, {"nbr_mask": bm}, {"reduce": "max"},
                   {"reduce": "min"}, {"attn": (z, z)}):
            with pytest.raises(ValueError, match="not built"):
                fn(adj, X, edge_weight=v, **kw)
        with pytest.raises(ValueError, match='reduce must be'):
            fn(adj, X, edge_weight=v, reduce="mean")             # an unknown word is named as such, not as "not built"
        with pytest.raises(ValueError):
            fn(adj, X, edge_weight=v[:-1])                       # a wrong length
        with pytest.raises(ValueError):
            fn(adj, X, edge_weight=v[:, None])
        with pytest.raises(TypeError):
            fn(adj, X, edge_weight=v.double())                   # a wrong dtype
        with pytest.raises(TypeError):
            fn(adj, X, edge_weight=g.values)                     # not a tensor
        with pytest.raises(ValueError):
            fn(adj, X, edge_weight=v.cpu())                      # a wrong device
        with pytest.raises(ValueError):
            fn(adj, X, edge_weight=torch.stack([v, v], 1)[:, 0])  # not contiguous
    # edge_values under validate=True
    row, col = tiled.edge_endpoints(adj)
    r64, c64, w = row.long(), col.long(), _dev(g.values)
    assert torch.equal(tiled.edge_values(adj, r64, c64, w), w)
    flip = torch.arange(g.nnz - 1, -1, -1, device="cuda")
    assert torch.equal(tiled.edge_values(adj, r64[flip], c64[flip], w[flip]), w)
    with pytest.raises(ValueError, match="more than one"):
        tiled.edge_values(adj, torch.cat([r64, r64[:1]]), torch.cat([c64, c64[:1]]), torch.cat([w, w[:1]]))
    with pytest.raises(ValueError, match="no stored cell"):
        tiled.edge_values(adj, torch.cat([r64, r64.new_tensor([5])]), torch.cat([c64, c64.new_tensor([0])]), torch.cat([w, w[:1]]))
    with pytest.raises(ValueError, match="no edge"):
        tiled.edge_values(adj, r64[1:], c64[1:], w[1:])
    lax = tiled.edge_values(adj, torch.cat([r64[1:], r64.new_tensor([5])]), torch.cat([c64[1:], c64.new_tensor([0])]), w, validate=False)
    assert lax[0] == 0 and torch.equal(lax[1:], w[:-1])
    with pytest.raises(ValueError):
        tiled.edge_values(adj, r64, c64, w[1:])
    with pytest.raises(TypeError):
        tiled.edge_values(adj, r64, c64, w.double())
    with pytest.raises(TypeError):
        tiled.edge_slots(adj, row, col)                          # int32 ids
    with pytest.raises(ValueError):
        tiled.tiledSDDMM(adj, X, X[:, :4].contiguous())


def test_gcnconv_with_edge_weight():
    torch = _torch()
    import QGTC
    from qgtc_ppopp22_amd import conv

    for n, reorder in ((129, False), (300, True)):
        g = graph(n, reorder)
        torch.manual_seed(n)
        layer = conv.GCNConv(12, 20, 7).cuda()
        X = _dev(g.X(12, special=False))
        ones, v = torch.ones(g.nnz, device="cuda"), _dev(g.values)
        assert same_bits(layer(g.adj, X, edge_weight=ones), layer(g.adj, X))
        h = QGTC.tiledAggregate(g.adj, torch.mm(g.adj.to_new(X), layer.W_in), edge_weight=v)
        want = g.adj.to_old(QGTC.tiledAggregate(g.adj, torch.mm(h, layer.W_out), edge_weight=v))
        assert same_bits(layer(g.adj, X, edge_weight=v), want)
        vg = v.clone().requires_grad_(True)
        layer(g.adj, X, edge_weight=vg).sum().backward()
        assert vg.grad is not None and layer.W_in.grad is not None
    g = graph(129)
    X, v = _dev(g.X(12, special=False)), _dev(g.values)
    for kw in ({"norm": "mean"}, {"norm": "sym"}, {"aggr": "max"}):
        with pytest.raises(ValueError, match="edge_endpoints"):
            conv.GCNConv(12, 20, 7, **kw).cuda()(g.adj, X, edge_weight=v)
    with pytest.raises(ValueError, match="edge_endpoints"):
        conv.GCNConv(12, 20, 7).cuda()(g.adj, X, edge_weight=v, nodes=torch.ones(g.n, dtype=torch.bool, device="cuda"))
