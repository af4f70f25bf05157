"""The float tiled products on the device (QGTC.tiledMMFloat on adj and adj.T, GCNConv_Qnt(float_out=True), and the two C-ABI entries
behind them) against the exact model of tests/tiled_float_model.py. The order of the adds is part of the contract, so every comparison
is bit for bit (a NaN equals a NaN), nothing is sampled and no tolerance is used."""
import ctypes

import numpy as np
import pytest

from tiled_float_model import (FLOAT_FORWARD_VARIANTS, FLOAT_TRANSPOSED_VARIANTS, aggregate_f32, float_chunks, float_variant,
                               neighbour_lists)
from tiled_model import aggregate, expected_floats, random_edges
from tiled_scaled_model import degrees, mean_scale, scaled

pytestmark = pytest.mark.gpu

CANARY = 64
NAN_WORD = 0x7FC00000                              # the float NaN torch.full writes
NO_EDGES = (np.zeros(0, np.int64), np.zeros(0, np.int64))

# N over every variant boundary of both launchers (forward 16 / 32 / 64 / 128 and the 256-column chunks, transposed 16 / 32 and the
# 64-column chunks), the unaligned rows 1, 3, 5, and up to 383; n rotates alongside
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


def _raw(torch, lib, adj, X, scale, transposed):
    """The C entry on `out` pre-filled with NaN and followed by CANARY words: (the n * N outputs, the canaries)."""
    n, N = X.shape
    out = torch.full((n * N + CANARY,), float("nan"), dtype=torch.float32, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    tail = (adj.n_tiles, n, X.data_ptr(), X.numel(), N, _ptr(scale), out.data_ptr(), n * N, st)
    if transposed:
        t = adj.T
        rc = lib.qgtc_tiledmm_f32_t(_ptr(t.col_ptr), _ptr(t.col_tile), _ptr(t.col_rb), _ptr(adj.tiles), *tail)
    else:
        rc = lib.qgtc_tiledmm_f32(_ptr(adj.row_ptr), _ptr(adj.kquad), _ptr(adj.tiles), *tail)
    assert rc == 0, rc
    got = out.cpu().numpy()
    return got[: n * N].reshape(n, N), got[n * N:]


# ---- 1. the sweep: every variant, both directions, three scales, both ways in -----------------------------------------------------------
def test_the_sweep_hits_every_variant():
    for transposed, variants in ((False, FLOAT_FORWARD_VARIANTS), (True, FLOAT_TRANSPOSED_VARIANTS)):
        hit = {}
        for _, N in SWEEP:
            hit.setdefault(float_variant(N, transposed), set()).add(N)
        assert sorted(hit) == sorted(variants)
        assert all(len(Ns) >= 2 for Ns in hit.values()), hit       # each at a ragged N and at its full width
        assert max(float_chunks(N, transposed) for _, N in SWEEP) >= 2
    for n in SWEEP_n:                                              # every n meets order-sensitive widths (N >= 16) in both kernels
        assert sum(1 for m, N in SWEEP if m == n and N >= 16) >= 2, n


@pytest.mark.parametrize("n,N", SWEEP, ids=[f"n{n}-N{N}" for n, N in SWEEP])
def test_every_variant_equals_the_model(qgtc, lib, n, N):
    import torch

    rng = np.random.default_rng(11 * n + N)
    src, dst = random_edges(rng, n, 6 * n + 5)
    X = rng.standard_normal((n, N)).astype(np.float32)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    dX = _dev(torch, X)
    degs = degrees(src, dst, n)
    for transposed in (False, True):
        a = adj.T if transposed else adj
        deg = degs[1 if transposed else 0]
        np.testing.assert_array_equal(a.degrees().cpu().numpy(), deg)
        scales = {"none": None, "mean": mean_scale(deg), "random": rng.uniform(2.0 ** -10, 4.0, n).astype(np.float32)}
        for kind, scale in scales.items():
            want = aggregate_f32(src, dst, n, X, transposed, scale)
            assert not np.isnan(want).any()
            if n >= 96 and not transposed:
                assert not want[32:64].any()       # the empty row block
            if n >= 512 and transposed:
                assert not want[128:256].any()     # the empty k-quad
            what = f"{'adj.T' if transposed else 'adj'} variant={float_variant(N, transposed)} scale={kind}"
            ds = None if scale is None else _dev(torch, scale)
            got = qgtc.tiledMMFloat(a, dX, ds)
            assert got.dtype == torch.float32 and got.shape == (n, N) and got.is_contiguous(), what
            assert_floats_identical(got.cpu().numpy(), want, what)
            raw, canaries = _raw(torch, lib, adj, dX, ds, transposed)
            assert_floats_identical(raw, want, what + " (C entry)")
            assert (canaries.view(np.uint32) == NAN_WORD).all(), what + " canaries"


# ---- 2. an adjacency without tiles ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,N", [(1, 1), (300, 24), (33, 130), (4097, 257)])
def test_an_empty_adjacency_gives_positive_zeros(qgtc, lib, n, N):
    """n_tiles = 0: through tiledMMFloat, and through the C entries with NULL index pointers. With a scale the zeros are multiplied
    like any sum (0 * inf is NaN)."""
    import torch

    rng = np.random.default_rng(n)
    adj = qgtc.pack_edges_tiled(_dev(torch, NO_EDGES[0]), _dev(torch, NO_EDGES[1]), n)
    assert adj.n_tiles == 0
    X = _dev(torch, rng.standard_normal((n, N)).astype(np.float32))
    scale = np.where(np.arange(n) % 3 == 0, np.inf, 2.0).astype(np.float32)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for transposed in (False, True):
        a = adj.T if transposed else adj
        got = qgtc.tiledMMFloat(a, X).cpu().numpy()
        assert (got.view(np.uint32) == 0).all(), transposed                    # +0.0f, not -0.0f
        with np.errstate(invalid="ignore"):
            want = np.zeros((n, N), np.float32) * scale[:, None]
        assert_floats_identical(qgtc.tiledMMFloat(a, X, _dev(torch, scale)).cpu().numpy(), want, f"scaled transposed={transposed}")
        out = torch.full((n * N + CANARY,), float("nan"), dtype=torch.float32, device="cuda")
        tail = (0, n, X.data_ptr(), X.numel(), N, None, out.data_ptr(), n * N, st)
        rc = lib.qgtc_tiledmm_f32_t(None, None, None, None, *tail) if transposed else lib.qgtc_tiledmm_f32(None, None, None, *tail)
        assert rc == 0
        raw = out.cpu().numpy().view(np.uint32)
        assert (raw[: n * N] == 0).all() and (raw[n * N:] == NAN_WORD).all(), transposed


# ---- 3. reordered adjacencies -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,N", [(97, 20), (1000, 64), (4097, 130)])
def test_reordered_adds_follow_the_new_ids(qgtc, n, N):
    """pack_edges_tiled(..., reorder=True): the expected value is the model on the relabelled edge list (rank[src], rank[dst]) with
    X[perm], moved back with rank. For integer X below 2^24 that is also the unreordered result."""
    import torch

    rng = np.random.default_rng(3 * n + N)
    src, dst = random_edges(rng, n, 6 * n + 5)
    X = rng.standard_normal((n, N)).astype(np.float32)
    Xi = rng.integers(0, 256, size=(n, N)).astype(np.float32)
    dsrc, ddst = _dev(torch, src), _dev(torch, dst)
    re, plain = qgtc.pack_edges_tiled(dsrc, ddst, n, reorder=True), qgtc.pack_edges_tiled(dsrc, ddst, n)
    assert re.perm is not None
    perm, rank = re.perm.cpu().numpy(), re.rank.cpu().numpy()
    if n >= 1000:                                  # below the community cap the renumbering may be the identity
        assert (perm != np.arange(n)).any()
    rsrc, rdst = rank[src], rank[dst]
    for transposed in (False, True):
        a, p = (re.T, plain.T) if transposed else (re, plain)
        deg_new = degrees(rsrc, rdst, n)[1 if transposed else 0]
        for kind, scale_new in (("none", None), ("mean", mean_scale(deg_new))):
            want = aggregate_f32(rsrc, rdst, n, X[perm], transposed, scale_new)[rank]
            ds = None if scale_new is None else a.mean_scale()
            got = a.to_old(qgtc.tiledMMFloat(a, a.to_new(_dev(torch, X)), ds))
            assert_floats_identical(got.cpu().numpy(), want, f"transposed={transposed} scale={kind}")
            ps = None if scale_new is None else p.mean_scale()
            got_i = a.to_old(qgtc.tiledMMFloat(a, a.to_new(_dev(torch, Xi)), ds))
            assert torch.equal(got_i.view(torch.int32), qgtc.tiledMMFloat(p, _dev(torch, Xi), ps).view(torch.int32)), (transposed, kind)


# ---- 4. isolation: a non-finite value reaches exactly the adjacent rows -----------------------------------------------------------------
@pytest.mark.parametrize("n,N", [(1000, 20), (4097, 70)])
def test_non_finite_inputs_reach_exactly_the_adjacent_rows(qgtc, n, N):
    import torch

    rng = np.random.default_rng(n + N)
    src, dst = random_edges(rng, n, 6 * n + 5)
    X = rng.standard_normal((n, N)).astype(np.float32)
    planted = [(n // 2, 0, np.nan), (n // 3, 1, np.inf), (5, 2, -np.inf), (n - 1, N - 1, np.nan), (40, 3, np.inf), (n // 3, 4, -np.inf)]
    for v, c, val in planted:
        X[v, c] = val
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    for transposed in (False, True):
        a = adj.T if transposed else adj
        out_row, nb, deg = neighbour_lists(src, dst, n, transposed)
        for scale in (None, mean_scale(deg)):
            want = aggregate_f32(src, dst, n, X, transposed, scale)
            bad = np.zeros((n, N), bool)
            for v, c, _ in planted:
                bad[out_row[nb == v], c] = True
            np.testing.assert_array_equal(~np.isfinite(want), bad)                  # the model's non-finite elements: these and no others
            assert bad.any(axis=0).sum() >= 4
            got = qgtc.tiledMMFloat(a, _dev(torch, X), None if scale is None else _dev(torch, scale)).cpu().numpy()
            np.testing.assert_array_equal(~np.isfinite(got), bad, err_msg=f"transposed={transposed}")
            assert_floats_identical(got, want, f"transposed={transposed} scaled={scale is not None}")


# ---- 5. against the bit kernels ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [1, 2, 8])
@pytest.mark.parametrize("n,N", [(97, 33), (1000, 64), (4097, 20)])
def test_integers_equal_the_bit_products(qgtc, n, N, w):
    """Integer X in 0 .. 2^w - 1 with sums below 2^24: tiledMMFloat(adj, X, s) == tiledMM2Int(adj, val2bit(X, w, True, False), N, w, s)."""
    import torch

    rng = np.random.default_rng(n * w + N)
    src, dst = random_edges(rng, n, 6 * n + 5)
    Xq = rng.integers(0, 2 ** w, size=(n, N))
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    X = _dev(torch, Xq.astype(np.float32))
    bits = qgtc.val2bit(X, w, True, False)
    for transposed in (False, True):
        a = adj.T if transposed else adj
        C = aggregate(src, dst, n, Xq, transposed)
        assert C.max() < 2 ** 24
        for s in (None, a.mean_scale()):
            got = qgtc.tiledMMFloat(a, X, s)
            assert torch.equal(got.view(torch.int32), qgtc.tiledMM2Int(a, bits, N, w, s).view(torch.int32)), (transposed, s is not None)
            if s is None:
                assert_floats_identical(got.cpu().numpy(), expected_floats(C))


def test_a_hub_sum_across_two_to_the_24(qgtc):
    """A hub row and a hub column of degree 66 000 over nodes that carry 255: the exact sum 16 830 000 is above 2^24 = 16 777 216. The bit
    route converts the exact integer (even, so representable); the float route adds 255 at a time and rounds every add past 2^24 to an
    even number. Here the two routes legitimately differ: each is compared with its own model, and the difference is asserted."""
    import torch

    n, N, d = 70000, 16, 66000
    hub_row, hub_col = n - 2, n - 1
    rng = np.random.default_rng(24)
    nb = np.arange(d, dtype=np.int64)
    s, t = rng.integers(0, n - 2, 2 * n), rng.integers(0, n - 2, 2 * n)
    src = np.concatenate([np.full(d, hub_row, np.int64), nb, s])
    dst = np.concatenate([nb, np.full(d, hub_col, np.int64), t])
    Xq = np.where(np.arange(n) < d, 255, 1)[:, None].repeat(N, axis=1)
    Xq[:d, 1] = rng.integers(0, 256, d)            # a column of mixed values
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    X = _dev(torch, Xq.astype(np.float32))
    bits = qgtc.val2bit(X, 8, True, False)
    for transposed, hub in ((False, hub_row), (True, hub_col)):
        a = adj.T if transposed else adj
        C = aggregate(src, dst, n, Xq, transposed)
        assert C[hub, 0] == 255 * d and C[hub, 0] > 2 ** 24
        want = aggregate_f32(src, dst, n, Xq.astype(np.float32), transposed)
        assert want[hub, 0] != np.float32(C[hub, 0])                                # the routes differ at the hub ...
        others = np.arange(n) != hub
        np.testing.assert_array_equal(want[others], expected_floats(C)[others])     # ... and nowhere else
        assert_floats_identical(qgtc.tiledMMFloat(a, X).cpu().numpy(), want, f"float route, transposed={transposed}")
        assert_floats_identical(qgtc.tiledMM2Int(a, bits, N, 8).cpu().numpy(), expected_floats(C), f"bit route, transposed={transposed}")


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
        s = a.mean_scale()
        first, again = qgtc.tiledMMFloat(a, X, s), qgtc.tiledMMFloat(a, X, s)
        assert torch.equal(first.view(torch.int32), again.view(torch.int32)), a.transposed


# ---- 7. the domain's upper end ----------------------------------------------------------------------------------------------------------
def test_the_largest_n(qgtc):
    """n = 2^23, the graph of test_tiled_scaled_gpu.test_degrees_at_the_largest_n (corners, the last row block, the last k-quad), N = 8."""
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
    dX = _dev(torch, X)
    for transposed in (False, True):
        a = adj.T if transposed else adj
        deg = degrees(src, dst, n)[1 if transposed else 0]
        assert deg[n - 1] >= 2 and deg.max() >= 3
        assert_floats_identical(qgtc.tiledMMFloat(a, dX).cpu().numpy(), aggregate_f32(src, dst, n, X, transposed), f"transposed={transposed}")
        assert_floats_identical(qgtc.tiledMMFloat(a, dX, a.mean_scale()).cpu().numpy(),
                                aggregate_f32(src, dst, n, X, transposed, mean_scale(deg)), f"mean, transposed={transposed}")


# ---- 8. the module ----------------------------------------------------------------------------------------------------------------------
def _model_forward(oracle, m, src, dst, n, X, transposed):
    """GCNConv_Qnt(float_out=True) layer by layer: the first layer as the oracle and the scaled model give it (exact integer sums,
    requant or the value quantiser of the mean), the float32 product h . W_out from the oracle's bitmm2int, the last aggregate from the
    float model."""
    from tiled_model import expected_bits

    f_in, hid, f_out, a, w = m.input_dim, m.hidden_dim, m.output_dim, m.act_bit, m.w_bit
    W_in = oracle.val2bit(m.W_in.detach().cpu().numpy(), w, True)
    W_out = oracle.val2bit(m.W_out.detach().cpu().numpy(), w, True)
    scale = mean_scale(degrees(src, dst, n)[1 if transposed else 0]) if m.aggr == "mean" else None
    bit_X = oracle.val2bit(X, a)
    t = oracle.bit2val(oracle.bitmm2bit(bit_X, W_in, n, f_in, hid, a, w, a, col=True), a, n, hid, col_major=True)
    C = aggregate(src, dst, n, t, transposed)
    bit_h = expected_bits(oracle, C, a) if scale is None else oracle.pack(oracle.quantize(scaled(C, scale), a), a)
    hw = oracle.bitmm2int(bit_h, W_out, n, hid, f_out, a, w)
    return aggregate_f32(src, dst, n, hw, transposed, scale), hw


@pytest.mark.parametrize("aggr", ["sum", "mean"])
@pytest.mark.parametrize("n", [200, 1213])
def test_module_float_out_equals_the_model(qgtc, oracle, n, aggr):
    import torch

    from qgtc_ppopp22_amd.conv import GCNConv_Qnt

    torch.manual_seed(0)
    rng = np.random.default_rng(n)
    src, dst = random_edges(rng, n, 8 * n)
    dsrc, ddst = _dev(torch, src), _dev(torch, dst)
    m = GCNConv_Qnt(48, 64, 10, w_bit=2, act_bit=3, aggr=aggr, float_out=True).cuda()
    with torch.no_grad():                          # sparse weights and features: X . W stays below requant's clamp, so the layers differ
        m.W_in.mul_((torch.rand_like(m.W_in) < 0.08).float())
        m.W_out.mul_((torch.rand_like(m.W_out) < 0.08).float())
    X = (torch.randn(n, 48, device="cuda") * 2 + 2) * (torch.rand(n, 48, device="cuda") < 0.15).float()
    adj, re = qgtc.pack_edges_tiled(dsrc, ddst, n), qgtc.pack_edges_tiled(dsrc, ddst, n, reorder=True)
    quantised = GCNConv_Qnt(48, 64, 10, w_bit=2, act_bit=3, aggr=aggr).cuda()
    quantised.load_state_dict(m.state_dict())
    for transposed in (False, True):
        want, hw = _model_forward(oracle, m, src, dst, n, X.cpu().numpy(), transposed)
        got = m(adj.T if transposed else adj, X)
        assert got.dtype == torch.float32 and got.shape == (n, 10)
        assert_floats_identical(got.cpu().numpy(), want, f"transposed={transposed}")
        assert len(np.unique(want)) > 16           # the case tells the layers apart: not the constant a saturated chain gives
        assert hw.max() > 7                        # class scores the requantised route would clamp to 2^act_bit - 1 ...
        assert not torch.equal(quantised(adj.T if transposed else adj, X), got)     # ... so the two routes differ here
        # the class scores are integers and the sums stay below 2^24, so every add is exact and the numbering does not show
        assert np.abs(want).max() < 2 ** 24
        got_re = m(re.T if transposed else re, X)
        assert torch.equal(got_re.view(torch.int32), got.view(torch.int32)), f"reordered, transposed={transposed}"


def test_module_default_is_unchanged_and_refusals(qgtc):
    import torch

    from qgtc_ppopp22_amd.conv import GCNConv_Qnt

    n = 400
    torch.manual_seed(0)
    src, dst = random_edges(np.random.default_rng(n), n, 8 * n)
    dsrc, ddst = _dev(torch, src), _dev(torch, dst)
    X = torch.randn(n, 48, device="cuda")
    adj = qgtc.pack_edges_tiled(dsrc, ddst, n)
    default = GCNConv_Qnt(48, 64, 10, w_bit=2, act_bit=3).cuda()
    assert default.float_out is False
    explicit = GCNConv_Qnt(48, 64, 10, w_bit=2, act_bit=3, float_out=False).cuda()
    explicit.load_state_dict(default.state_dict())
    want = default((dsrc, ddst, n), X)             # the edge-list route: no tiled kernel involved
    assert torch.equal(default(adj, X), want) and torch.equal(explicit(adj, X), want) and torch.equal(explicit((dsrc, ddst, n), X), want)
    fl = GCNConv_Qnt(48, 64, 10, w_bit=2, act_bit=3, float_out=True).cuda()
    with pytest.raises(NotImplementedError, match="pack_edges_tiled"):
        fl((dsrc, ddst, n), X)
    with pytest.raises(NotImplementedError, match="pack_edges_tiled"):
        fl(torch.zeros(n, n, device="cuda"), X)
    assert fl(adj, X).shape == (n, 10)


# ---- 9. Python argument refusals --------------------------------------------------------------------------------------------------------
def test_operand_refusals(qgtc):
    import torch

    n, N = 100, 8
    src, dst = random_edges(np.random.default_rng(8), n, 6 * n)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    good = torch.ones(n, N, dtype=torch.float32, device="cuda")
    bad = [(TypeError, "float64", good.double()), (TypeError, "float16", good.half()), (TypeError, "int32", good.to(torch.int32)),
           (TypeError, "ndarray", np.ones((n, N), np.float32)), (TypeError, "list", [[1.0] * N] * n),
           (ValueError, rf"\[{n - 1}, {N}\]", good[:-1].contiguous()), (ValueError, rf"\[{n}\]", good[:, 0].contiguous()),
           (ValueError, rf"\[{n}, {N}, 1\]", good[:, :, None].contiguous()), (ValueError, rf"\[{n}, 0\]", good[:, :0]),
           (ValueError, "cpu", good.cpu()),
           (ValueError, "strides", torch.ones(n, 2 * N, dtype=torch.float32, device="cuda")[:, ::2]),
           (ValueError, "strides", torch.ones(N, n, dtype=torch.float32, device="cuda").t())]
    for a in (adj, adj.T):
        for exc, match, x in bad:
            with pytest.raises(exc, match=match):
                qgtc.tiledMMFloat(a, x)
        with pytest.raises(TypeError):
            qgtc.tiledMMFloat(a, good, row_scale=torch.ones(n, dtype=torch.float64, device="cuda"))
        with pytest.raises(ValueError):
            qgtc.tiledMMFloat(a, good, row_scale=torch.ones(n + 1, dtype=torch.float32, device="cuda"))
        assert qgtc.tiledMMFloat(a, good, row_scale=torch.ones(n, dtype=torch.float32, device="cuda")).shape == (n, N)
    with pytest.raises(TypeError):
        qgtc.tiledMMFloat((adj.row_ptr, adj.kquad, adj.tiles), good)
    assert "tiledMMFloat" in qgtc.__dict__ and "tiledMMFloat" in __import__("qgtc_ppopp22_amd.tiled", fromlist=["x"]).__all__
