"""The source-scaled float tiled products on the device (QGTC.tiledMMFloat(adj, X, row_scale, src_scale) on adj and adj.T, the C-ABI
entries qgtc_tiledmm_f32_src / _t_src / qgtc_tiled_inv_sqrt_degree behind it, TiledAdjacency.sym_scale, QGTC.tiledAggregate and its
backward, conv.GCNConv(norm=)) against the exact model of tests/tiled_sym_model.py. The order of the adds and the two roundings per term
are part of the contract, so every comparison with the model is bit for bit (a NaN equals a NaN), nothing is sampled and no tolerance
is used; the only bound is the derived one against float64 autograd."""
import ctypes

import numpy as np
import pytest

from tiled_float_model import FLOAT_FORWARD_VARIANTS, FLOAT_TRANSPOSED_VARIANTS, aggregate_f32, float_variant, neighbour_lists
from tiled_model import random_edges, set_cells
from tiled_scaled_model import degrees
from tiled_sym_model import add_self_loops, aggregate_f32_src, error_bound, inv_sqrt_degree

pytestmark = pytest.mark.gpu

CANARY = 64
NAN_WORD = 0x7FC00000                              # the float NaN torch.full writes
NO_EDGES = (np.zeros(0, np.int64), np.zeros(0, np.int64))

# N over every variant boundary of both launchers (forward 16 / 32 / 64 / 128 and the 256-column chunks, transposed 16 / 32 and the
# 64-column chunks), the unaligned rows 1, 3, 5, and up to 383; n rotates alongside (the sweep of tests/test_tiled_float_gpu.py)
SWEEP_N = [1, 3, 5, 15, 16, 17, 20, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 383]
SWEEP_n = [1, 31, 97, 1000, 4097]
SWEEP = [(SWEEP_n[(2 * i + 3) % 5], N) for i, N in enumerate(SWEEP_N)]


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def assert_floats_identical(got, want, what=""):
    """Bit for bit (so -0.0 is not 0.0), except that any NaN equals any NaN."""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    np.testing.assert_array_equal(gn, wn, err_msg=f"{what}: NaN positions")
    np.testing.assert_array_equal(got.view(np.uint32)[~gn], want.view(np.uint32)[~wn], err_msg=what)


@pytest.fixture(scope="module")
def lib():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    from qgtc_ppopp22_amd import cabi

    return cabi.load()


def _raw(torch, lib, adj, X, scale, src_scale, transposed):
    """The C entry on `out` pre-filled with NaN and followed by CANARY words: (the n * N outputs, the canaries)."""
    n, N = X.shape
    out = torch.full((n * N + CANARY,), float("nan"), dtype=torch.float32, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    tail = (adj.n_tiles, n, X.data_ptr(), X.numel(), N, _ptr(scale), _ptr(src_scale), out.data_ptr(), n * N, st)
    if transposed:
        t = adj.T
        rc = lib.qgtc_tiledmm_f32_t_src(_ptr(t.col_ptr), _ptr(t.col_tile), _ptr(t.col_rb), _ptr(adj.tiles), *tail)
    else:
        rc = lib.qgtc_tiledmm_f32_src(_ptr(adj.row_ptr), _ptr(adj.kquad), _ptr(adj.tiles), *tail)
    assert rc == 0, rc
    got = out.cpu().numpy()
    return got[: n * N].reshape(n, N), got[n * N:]


def _scale_pairs(rng, src, dst, n, transposed):
    """kind -> (row scale, source scale) on this view: the symmetric normalisation, random factors of both signs, and specials."""
    out_deg, in_deg = degrees(src, dst, n)
    r_deg, c_deg = (in_deg, out_deg) if transposed else (out_deg, in_deg)
    special = rng.uniform(0.5, 2.0, n).astype(np.float32)
    pick = rng.random(n)
    for k, v in enumerate((np.inf, -np.inf, np.nan, -0.0, 0.0)):
        special[(pick >= 0.02 * k) & (pick < 0.02 * (k + 1))] = v
    return {"sym": (inv_sqrt_degree(r_deg), inv_sqrt_degree(c_deg)),
            "random": (rng.uniform(2.0 ** -10, 4.0, n).astype(np.float32), rng.uniform(-4.0, 4.0, n).astype(np.float32)),
            "specials": (special[::-1].copy(), special)}


# ---- 1. the sweep: every variant, both directions, three pairs of scales, source scale alone and with a row scale, both ways in --------
def test_the_sweep_hits_every_variant():
    for transposed, variants in ((False, FLOAT_FORWARD_VARIANTS), (True, FLOAT_TRANSPOSED_VARIANTS)):
        hit = {}
        for _, N in SWEEP:
            hit.setdefault(float_variant(N, transposed), set()).add(N)
        assert sorted(hit) == sorted(variants)
        assert all(len(Ns) >= 2 for Ns in hit.values()), hit
    for n in SWEEP_n:
        assert sum(1 for m, N in SWEEP if m == n and N >= 16) >= 2, n


@pytest.mark.parametrize("n,N", SWEEP, ids=[f"n{n}-N{N}" for n, N in SWEEP])
def test_every_variant_equals_the_model(qgtc, lib, n, N):
    import torch

    rng = np.random.default_rng(13 * n + N)
    src, dst = random_edges(rng, n, 6 * n + 5)
    X = rng.standard_normal((n, N)).astype(np.float32)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    dX = _dev(torch, X)
    ones = torch.ones(n, dtype=torch.float32, device="cuda")
    for transposed in (False, True):
        a = adj.T if transposed else adj
        view = f"{'adj.T' if transposed else 'adj'} variant={float_variant(N, transposed)}"
        plain = qgtc.tiledMMFloat(a, dX)
        assert_floats_identical(plain.cpu().numpy(), aggregate_f32(src, dst, n, X, transposed), view + " no scales")
        # src_scale=None is the parent call; a source scale of ones gives the unscaled bits (1 * x is exact)
        assert torch.equal(qgtc.tiledMMFloat(a, dX, None, None).view(torch.int32), plain.view(torch.int32)), view
        assert torch.equal(qgtc.tiledMMFloat(a, dX, src_scale=ones).view(torch.int32), plain.view(torch.int32)), view + " ones"
        raw, canaries = _raw(torch, lib, adj, dX, None, None, transposed)              # the C entry with src_scale NULL
        assert_floats_identical(raw, plain.cpu().numpy(), view + " (C entry, NULL src_scale)")
        assert (canaries.view(np.uint32) == NAN_WORD).all()
        for kind, (r, c) in _scale_pairs(rng, src, dst, n, transposed).items():
            dc = _dev(torch, c)
            with np.errstate(invalid="ignore", over="ignore"):
                pre = _dev(torch, c[:, None] * X)                                       # the route without the feature
            for scale in (None, r):
                what = f"{view} scales={kind} row_scale={scale is not None}"
                want = aggregate_f32_src(src, dst, n, X, transposed, scale, c)
                if kind != "specials":
                    assert not np.isnan(want).any()
                ds = None if scale is None else _dev(torch, scale)
                got = qgtc.tiledMMFloat(a, dX, ds, dc)
                assert got.dtype == torch.float32 and got.shape == (n, N) and got.is_contiguous(), what
                assert_floats_identical(got.cpu().numpy(), want, what)
                assert_floats_identical(qgtc.tiledMMFloat(a, pre, ds).cpu().numpy(), want, what + " (pre-multiplied route)")
                raw, canaries = _raw(torch, lib, adj, dX, ds, dc, transposed)
                assert_floats_identical(raw, want, what + " (C entry)")
                assert (canaries.view(np.uint32) == NAN_WORD).all(), what + " canaries"


# ---- 2. an adjacency without tiles ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,N", [(1, 1), (300, 24), (33, 130), (4097, 257)])
def test_an_empty_adjacency_gives_positive_zeros(qgtc, lib, n, N):
    """n_tiles = 0: no term is formed, so a source scale of NaN or inf changes nothing; the row scale multiplies the zeros as ever."""
    import torch

    rng = np.random.default_rng(n)
    adj = qgtc.pack_edges_tiled(_dev(torch, NO_EDGES[0]), _dev(torch, NO_EDGES[1]), n)
    assert adj.n_tiles == 0
    X = _dev(torch, rng.standard_normal((n, N)).astype(np.float32))
    c = _dev(torch, np.where(np.arange(n) % 2 == 0, np.nan, np.inf).astype(np.float32))
    scale = np.where(np.arange(n) % 3 == 0, np.inf, 2.0).astype(np.float32)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for transposed in (False, True):
        a = adj.T if transposed else adj
        got = qgtc.tiledMMFloat(a, X, src_scale=c).cpu().numpy()
        assert (got.view(np.uint32) == 0).all(), transposed                    # +0.0f, not -0.0f
        with np.errstate(invalid="ignore"):
            want = np.zeros((n, N), np.float32) * scale[:, None]
        assert_floats_identical(qgtc.tiledMMFloat(a, X, _dev(torch, scale), c).cpu().numpy(), want, f"scaled transposed={transposed}")
        out = torch.full((n * N + CANARY,), float("nan"), dtype=torch.float32, device="cuda")
        tail = (0, n, X.data_ptr(), X.numel(), N, None, c.data_ptr(), out.data_ptr(), n * N, st)
        rc = lib.qgtc_tiledmm_f32_t_src(None, None, None, None, *tail) if transposed else lib.qgtc_tiledmm_f32_src(None, None, None, *tail)
        assert rc == 0
        raw = out.cpu().numpy().view(np.uint32)
        assert (raw[: n * N] == 0).all() and (raw[n * N:] == NAN_WORD).all(), transposed
        assert (a.sym_scale().cpu().numpy().view(np.uint32) == 0).all()         # degree 0 everywhere: +0


# ---- 3. reordered adjacencies -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,N", [(97, 20), (1000, 64), (4097, 130)])
def test_reordered_adds_follow_the_new_ids(qgtc, n, N):
    """pack_edges_tiled(..., reorder=True): the expected value is the model on the relabelled edge list (rank[src], rank[dst]) with
    X[perm] and the scales of the relabelled graph, moved back with rank."""
    import torch

    rng = np.random.default_rng(5 * n + N)
    src, dst = random_edges(rng, n, 6 * n + 5)
    X = rng.standard_normal((n, N)).astype(np.float32)
    re = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n, reorder=True)
    assert re.perm is not None
    perm, rank = re.perm.cpu().numpy(), re.rank.cpu().numpy()
    if n >= 1000:
        assert (perm != np.arange(n)).any()
    rsrc, rdst = rank[src], rank[dst]
    out_deg, in_deg = degrees(rsrc, rdst, n)
    for transposed in (False, True):
        a = re.T if transposed else re
        r, c = (inv_sqrt_degree(in_deg), inv_sqrt_degree(out_deg)) if transposed else (inv_sqrt_degree(out_deg), inv_sqrt_degree(in_deg))
        assert_floats_identical(a.sym_scale().cpu().numpy(), r, f"sym_scale transposed={transposed}")
        want = aggregate_f32_src(rsrc, rdst, n, X[perm], transposed, r, c)[rank]
        got = a.to_old(qgtc.tiledMMFloat(a, a.to_new(_dev(torch, X)), a.sym_scale(), a.T.sym_scale()))
        assert_floats_identical(got.cpu().numpy(), want, f"transposed={transposed}")


# ---- 4. isolation: a NaN in src_scale[v] reaches exactly the rows adjacent to v ------------------------------------------------------------
@pytest.mark.parametrize("n,N", [(1000, 20), (4097, 70)])
def test_a_nan_factor_reaches_exactly_the_adjacent_rows(qgtc, n, N):
    import torch

    rng = np.random.default_rng(n + N)
    src, dst = random_edges(rng, n, 6 * n + 5)
    X = rng.standard_normal((n, N)).astype(np.float32)
    c = rng.uniform(0.5, 2.0, n).astype(np.float32)
    planted = [n // 2, n // 3, 5, n - 1, 40]
    c[planted] = np.nan
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    for transposed in (False, True):
        a = adj.T if transposed else adj
        out_row, nb, deg = neighbour_lists(src, dst, n, transposed)
        bad = np.zeros(n, bool)
        bad[out_row[np.isin(nb, planted)]] = True
        assert 0 < bad.sum() < n
        for scale in (None, rng.uniform(0.5, 2.0, n).astype(np.float32)):
            want = aggregate_f32_src(src, dst, n, X, transposed, scale, c)
            np.testing.assert_array_equal(np.isnan(want), np.repeat(bad[:, None], N, axis=1))     # whole rows, these and no others
            got = qgtc.tiledMMFloat(a, _dev(torch, X), None if scale is None else _dev(torch, scale), _dev(torch, c)).cpu().numpy()
            np.testing.assert_array_equal(np.isnan(got), np.repeat(bad[:, None], N, axis=1), err_msg=f"transposed={transposed}")
            assert_floats_identical(got, want, f"transposed={transposed} scaled={scale is not None}")


# ---- 5. the inverse square roots ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 31, 97, 1000, 4097])
def test_sym_scale_equals_the_model_and_is_shared(qgtc, n):
    import torch

    rng = np.random.default_rng(70 + n)
    src, dst = random_edges(rng, n, 6 * n + 5)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    out_deg, in_deg = degrees(src, dst, n)
    got_out, got_in = adj.sym_scale(), adj.T.sym_scale()
    assert got_out.dtype == torch.float32 and got_out.shape == (n,) and got_out.is_contiguous()
    assert_floats_identical(got_out.cpu().numpy(), inv_sqrt_degree(out_deg), "out")
    assert_floats_identical(got_in.cpu().numpy(), inv_sqrt_degree(in_deg), "in")
    assert adj.sym_scale() is got_out and adj.T.sym_scale() is got_in and adj.T.T.sym_scale() is got_out      # cached, one pair for both views
    fresh = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    assert torch.equal(fresh.T.sym_scale(), got_in) and torch.equal(fresh.sym_scale(), got_out)                 # asked on adj.T first


def test_inverse_square_root_of_every_degree(lib):
    """qgtc_tiled_inv_sqrt_degree on deg = 0 .. 2^23 - 1 and on 2^23 (every degree of the domain), NaN-filled output with canaries: both
    roundings are IEEE's, so the words equal NumPy's."""
    import torch

    n = 1 << 23
    deg = np.arange(n, dtype=np.int32)
    deg[5] = n                                     # the largest degree takes the place of one small one (checked below on its own)
    d = _dev(torch, deg)
    out = torch.full((n + CANARY,), float("nan"), dtype=torch.float32, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.qgtc_tiled_inv_sqrt_degree(d.data_ptr(), n, out.data_ptr(), st) == 0
    got = out.cpu().numpy()
    np.testing.assert_array_equal(got[:n].view(np.uint32), inv_sqrt_degree(deg).view(np.uint32))
    assert (got[n:].view(np.uint32) == NAN_WORD).all()
    assert got[0].view(np.uint32) == 0 and got[1] == 1.0 and got[4] == 0.5 and got[5].view(np.uint32) == 0x39B504F3
    small = _dev(torch, np.array([5], dtype=np.int32))
    out.fill_(float("nan"))
    assert lib.qgtc_tiled_inv_sqrt_degree(small.data_ptr(), 1, out.data_ptr(), st) == 0
    assert out[:2].cpu().numpy().view(np.uint32).tolist() == [int(inv_sqrt_degree(np.array([5])).view(np.uint32)[0]), NAN_WORD]   # n = 1 writes one


def test_sym_scale_at_the_largest_n(qgtc):
    """n = 2^23, the corner graph of tests/test_tiled_float_gpu.py: sym_scale in both directions and one normalised product, N = 8."""
    import torch

    n, N = 1 << 23, 8
    rng = np.random.default_rng(23)
    corner = np.array([[0, 0], [0, n - 1], [n - 1, 0], [n - 1, n - 1], [n - 1, n - 1], [n - 1, n - 1],
                       [n - 2, n - 3], [n - 2, n - 3], [n - 32, n - 128], [n - 31, 5], [127, n - 129]], dtype=np.int64)
    last = np.stack([rng.integers(n - 32, n, 300), rng.integers(n - 128, n, 300)], axis=1)
    spread = rng.integers(0, n, size=(20000, 2))
    e = np.concatenate([corner, last, spread, spread[:500], spread[:100]])
    src, dst = np.ascontiguousarray(e[:, 0]), np.ascontiguousarray(e[:, 1])
    X = rng.standard_normal((n, N), dtype=np.float32)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    out_deg, in_deg = degrees(src, dst, n)
    r, c = inv_sqrt_degree(out_deg), inv_sqrt_degree(in_deg)
    assert_floats_identical(adj.sym_scale().cpu().numpy(), r, "out")
    assert_floats_identical(adj.T.sym_scale().cpu().numpy(), c, "in")
    dX = _dev(torch, X)
    assert_floats_identical(qgtc.tiledMMFloat(adj, dX, adj.sym_scale(), adj.T.sym_scale()).cpu().numpy(),
                            aggregate_f32_src(src, dst, n, X, False, r, c), "forward")
    assert_floats_identical(qgtc.tiledMMFloat(adj.T, dX, adj.T.sym_scale(), adj.sym_scale()).cpu().numpy(),
                            aggregate_f32_src(src, dst, n, X, True, c, r), "transposed")


# ---- 6. determinism ---------------------------------------------------------------------------------------------------------------------
def test_two_launches_give_identical_bits(qgtc):
    import torch

    n, N = 4097, 96
    rng = np.random.default_rng(6)
    src, dst = random_edges(rng, n, 6 * n + 5)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    assert int(adj.degrees().max()) > 1000 and int(adj.T.degrees().max()) > 1000    # a hub in each direction
    X = _dev(torch, rng.standard_normal((n, N)).astype(np.float32))
    for a in (adj, adj.T):
        r, c = a.sym_scale(), a.T.sym_scale()
        first, again = qgtc.tiledMMFloat(a, X, r, c), qgtc.tiledMMFloat(a, X, r, c)
        assert torch.equal(first.view(torch.int32), again.view(torch.int32)), a.transposed


# ---- 7. autograd ------------------------------------------------------------------------------------------------------------------------
def _dense(src, dst, n, transposed):
    A = np.zeros((n, n))
    cells = set_cells(src, dst, n)
    A[cells // n, cells % n] = 1.0
    return A.T if transposed else A


@pytest.mark.parametrize("kind", ["sym", "random", "row only", "src only", "none"])
@pytest.mark.parametrize("n,N", [(97, 20), (1000, 64), (2049, 130)])
def test_the_gradient_is_the_swapped_transposed_product(qgtc, n, N, kind):
    """Y = diag(r) A diag(c) X, so dX = diag(c) A^T diag(r) dY: X.grad from tiledAggregate equals the MODEL of that product (the other
    direction, the two scales swapped) bit for bit, on adj and adj.T, and lies within the derived bound (d + 2) 2^-24 |c| sum |r dY| of
    the gradient torch's own autograd gives for the dense float64 expression."""
    import torch

    rng = np.random.default_rng(7 * n + N)
    src, dst = random_edges(rng, n, 6 * n + 5)
    X = rng.standard_normal((n, N)).astype(np.float32)
    dY = rng.standard_normal((n, N)).astype(np.float32)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    for transposed in (False, True):
        a = adj.T if transposed else adj
        pairs = _scale_pairs(rng, src, dst, n, transposed)
        r, c = pairs["random" if kind in ("row only", "src only") else kind] if kind != "none" else (None, None)
        r, c = (None if kind == "src only" else r), (None if kind == "row only" else c)
        dr, dc = (None if r is None else _dev(torch, r)), (None if c is None else _dev(torch, c))
        dX = _dev(torch, X).requires_grad_(True)
        Y = qgtc.tiledAggregate(a, dX, dr, dc)
        assert Y.requires_grad
        assert_floats_identical(Y.detach().cpu().numpy(), aggregate_f32_src(src, dst, n, X, transposed, r, c), "forward")
        Y.backward(_dev(torch, dY))
        want = aggregate_f32_src(src, dst, n, dY, not transposed, c, r)
        assert_floats_identical(dX.grad.cpu().numpy(), want, f"X.grad transposed={transposed} {kind}")
        # float64 autograd of the dense expression, on the host
        A = torch.from_numpy(_dense(src, dst, n, transposed))
        X64 = torch.from_numpy(X.astype(np.float64)).requires_grad_(True)
        r64 = torch.ones(n, dtype=torch.float64) if r is None else torch.from_numpy(r.astype(np.float64))
        c64 = torch.ones(n, dtype=torch.float64) if c is None else torch.from_numpy(c.astype(np.float64))
        (r64[:, None] * (A @ (c64[:, None] * X64))).backward(torch.from_numpy(dY.astype(np.float64)))
        exact, bound = error_bound(src, dst, n, dY, not transposed, c, r)
        ref = X64.grad.numpy()
        assert np.abs(ref - exact).max() <= 1e-9 * max(1.0, np.abs(exact).max())      # the two float64 statements of the gradient agree
        err = np.abs(dX.grad.cpu().numpy().astype(np.float64) - ref)
        assert (err <= bound * (1 + 2.0 ** -20)).all(), float((err / np.maximum(bound, 1e-300)).max())   # 2^-20: the float64 reference's own error


def test_the_gradient_on_a_reordered_adjacency_and_through_a_view(qgtc):
    """to_new / to_old are index_select and differentiate by themselves: the gradient for X in the edge list's numbering is the model on
    the relabelled graph, moved there and back. A non-contiguous dY (an expanded scalar from sum()) is made contiguous."""
    import torch

    n, N = 1000, 40
    rng = np.random.default_rng(77)
    src, dst = random_edges(rng, n, 6 * n + 5)
    X = rng.standard_normal((n, N)).astype(np.float32)
    dY = rng.standard_normal((n, N)).astype(np.float32)
    re = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n, reorder=True)
    perm, rank = re.perm.cpu().numpy(), re.rank.cpu().numpy()
    assert (perm != np.arange(n)).any()
    rsrc, rdst = rank[src], rank[dst]
    out_deg, in_deg = degrees(rsrc, rdst, n)
    for transposed in (False, True):
        a = re.T if transposed else re
        r, c = (inv_sqrt_degree(in_deg), inv_sqrt_degree(out_deg)) if transposed else (inv_sqrt_degree(out_deg), inv_sqrt_degree(in_deg))
        dX = _dev(torch, X).requires_grad_(True)
        Y = a.to_old(qgtc.tiledAggregate(a, a.to_new(dX), a.sym_scale(), a.T.sym_scale()))
        Y.backward(_dev(torch, dY))
        want = aggregate_f32_src(rsrc, rdst, n, dY[perm], not transposed, c, r)[rank]
        assert_floats_identical(dX.grad.cpu().numpy(), want, f"transposed={transposed}")
        dX2 = _dev(torch, X).requires_grad_(True)
        qgtc.tiledAggregate(a, dX2, a.sym_scale(), a.T.sym_scale()).sum().backward()      # dY = ones, expanded: stride 0
        want1 = aggregate_f32_src(rsrc, rdst, n, np.ones((n, N), np.float32), not transposed, c, r)
        assert_floats_identical(dX2.grad.cpu().numpy(), want1, f"sum() transposed={transposed}")
    no_grad = qgtc.tiledAggregate(re, _dev(torch, X), re.sym_scale(), re.T.sym_scale())
    assert not no_grad.requires_grad
    with pytest.raises(ValueError, match="src_scale must not require a gradient"):
        qgtc.tiledAggregate(re, _dev(torch, X), None, re.sym_scale().clone().requires_grad_(True))


# ---- 8. the module ----------------------------------------------------------------------------------------------------------------------
def _graph_with_loops(torch, qgtc, n, seed, reorder=False):
    rng = np.random.default_rng(seed)
    s, d = random_edges(rng, n, 4 * n)
    s, d = np.concatenate([s, d, np.arange(0, n, 7)]), np.concatenate([d, s, np.arange(0, n, 7)])     # symmetric, some loops already there
    ds, dd = qgtc.add_self_loops(_dev(torch, s), _dev(torch, d), n)
    ms, md = add_self_loops(s, d, n)
    np.testing.assert_array_equal(ds.cpu().numpy(), ms)
    np.testing.assert_array_equal(dd.cpu().numpy(), md)
    return ms, md, qgtc.pack_edges_tiled(ds, dd, n, reorder=reorder)


@pytest.mark.parametrize("norm", [None, "mean", "sym"])
def test_module_forward_is_two_aggregates(qgtc, norm):
    """GCNConv(norm) on a TiledAdjacency: agg(agg(X W_in) W_out), each aggregate bit for bit the model on the matrix it was given; on a
    reordered adjacency X goes to its numbering and the result comes back."""
    import torch

    from qgtc_ppopp22_amd.conv import GCNConv

    n = 600
    torch.manual_seed(0)
    src, dst, adj = _graph_with_loops(torch, qgtc, n, 1)
    out_deg, in_deg = degrees(src, dst, n)
    assert (out_deg >= 1).all() and np.array_equal(out_deg, in_deg)                  # symmetric, every node has its loop
    m = GCNConv(24, 32, 7, norm=norm).cuda()
    X = torch.randn(n, 24, device="cuda")
    for transposed in (False, True):
        a = adj.T if transposed else adj
        r_deg, c_deg = (in_deg, out_deg) if transposed else (out_deg, in_deg)
        with np.errstate(divide="ignore"):
            r, c = {None: (None, None), "mean": ((np.float32(1) / r_deg.astype(np.float32)), None),
                    "sym": (inv_sqrt_degree(r_deg), inv_sqrt_degree(c_deg))}[norm]
        got = m(a, X)
        assert got.shape == (n, 7) and got.requires_grad
        xw = torch.mm(X, m.W_in).detach()
        h = aggregate_f32_src(src, dst, n, xw.cpu().numpy(), transposed, r, c)
        hw = torch.mm(_dev(torch, h), m.W_out).detach()
        assert_floats_identical(got.detach().cpu().numpy(), aggregate_f32_src(src, dst, n, hw.cpu().numpy(), transposed, r, c),
                                f"norm={norm} transposed={transposed}")
    re = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n, reorder=True)
    row, sc = {None: (None, None), "mean": (re.mean_scale(), None), "sym": (re.sym_scale(), re.T.sym_scale())}[norm]
    by_hand = re.to_old(qgtc.tiledMMFloat(re, torch.mm(qgtc.tiledMMFloat(re, torch.mm(re.to_new(X), m.W_in).detach().contiguous(), row, sc),
                                                        m.W_out).detach().contiguous(), row, sc))
    assert torch.equal(m(re, X).detach().view(torch.int32), by_hand.view(torch.int32))
    dense = GCNConv(24, 32, 7).cuda()
    A = torch.rand(50, 50, device="cuda")
    Xs = X[:50]
    assert torch.equal(dense(A, Xs), torch.mm(A, torch.mm(torch.mm(A, torch.mm(Xs, dense.W_in)), dense.W_out)))     # what it did
    with pytest.raises(NotImplementedError, match="pack_edges_tiled"):
        GCNConv(24, 32, 7, norm="sym").cuda()(A, Xs)


def _train(torch, qgtc, adj, X, target, steps):
    from qgtc_ppopp22_amd.conv import GCNConv

    torch.manual_seed(3)
    m = GCNConv(16, 32, 5, norm="sym")
    with torch.no_grad():
        m.W_in.mul_(0.3)
        m.W_out.mul_(0.3)
    m = m.cuda()
    opt = torch.optim.SGD(m.parameters(), lr=0.5)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        loss = torch.nn.functional.cross_entropy(m(adj, X), target)
        loss.backward()
        assert m.W_in.grad is not None and m.W_out.grad is not None and torch.isfinite(m.W_in.grad).all()
        opt.step()
        losses.append(float(loss.detach()))
    return losses, m.W_in.detach().clone(), m.W_out.detach().clone()


@pytest.mark.parametrize("reorder", [False, True])
def test_training_lowers_the_loss_and_repeats_bit_for_bit(qgtc, reorder):
    """GCNConv(norm="sym") on an add_self_loops graph: a few SGD steps on a fixed seed lower the loss, and two runs end with identical
    weight bits (the aggregates, forwards and backwards, are functions of their inputs alone; torch.mm is run-to-run deterministic on
    one device)."""
    import torch

    n = 1200
    src, dst, adj = _graph_with_loops(torch, qgtc, n, 9, reorder)
    g = torch.Generator().manual_seed(5)
    X = torch.randn(n, 16, generator=g).cuda()
    target = (X[:, :5] + 0.1 * torch.randn(n, 5, generator=g).cuda()).argmax(dim=1)       # the class is readable from the node's own features
    first = _train(torch, qgtc, adj, X, target, 8)
    again = _train(torch, qgtc, adj, X, target, 8)
    assert first[0][-1] < first[0][0], first[0]
    assert min(first[0][1:]) < first[0][0] and all(np.isfinite(first[0]))
    assert first[0] == again[0]
    assert torch.equal(first[1].view(torch.int32), again[1].view(torch.int32))
    assert torch.equal(first[2].view(torch.int32), again[2].view(torch.int32))
