"""The scaled tiled products and the degrees on the device (QGTC.tiledMM2Bit / tiledMM2Int with row_scale, TiledAdjacency.degrees /
mean_scale, GCNConv_Qnt(aggr="mean"), and the five C-ABI entries behind them) against the exact model of tests/tiled_scaled_model.py.
Every comparison is exact: bits word for word, floats bit for bit (a NaN equals a NaN), nothing sampled."""
import ctypes

import numpy as np
import pytest

from helpers import to_np_u32
from qgtc_ppopp22_amd.shapes import P8, S128
from test_tiled_variants_gpu import SWEEP
from tiled_model import aggregate, expected_bits, expected_floats, random_edges, variant
from tiled_scaled_model import degrees, expected_bits_scaled, mean_scale, scaled

pytestmark = pytest.mark.gpu

CANARY = 64
POISON_BITS = -0x5A5A5A5B                          # 0xA5A5A5A5 as int32
NAN_WORD = 0x7FC00000                              # the float NaN torch.full writes
SPECIALS = np.array([0.0, -0.0, 1.0, 0.5, -1.0, np.inf, -np.inf, np.nan, 2.0 ** 20, 2.0 ** -20], dtype=np.float32)
NO_EDGES = (np.zeros(0, np.int64), np.zeros(0, np.int64))


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits_of(qgtc, torch, Xq, w):
    """X in the cols layout, from the quantised features."""
    return qgtc.val2bit(torch.from_numpy(np.ascontiguousarray(Xq, dtype=np.float32)).cuda(), w, True, False)


def assert_floats_identical(got, want, what=""):
    """Bit for bit (so -0.0 is not 0.0), except that any NaN equals any NaN."""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    np.testing.assert_array_equal(gn, wn, err_msg=f"{what}: NaN positions")
    np.testing.assert_array_equal(got.view(np.uint32)[~gn], want.view(np.uint32)[~wn], err_msg=what)


def _scales(rng, n, deg):
    """The three row scales of the sweep: the mean scale, random positive floats in [2^-10, 4), the special values cycling over the rows."""
    return {"mean": mean_scale(deg), "random": rng.uniform(2.0 ** -10, 4.0, n).astype(np.float32), "special": SPECIALS[np.arange(n) % SPECIALS.size]}


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


@pytest.fixture(scope="module")
def lib():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    from qgtc_ppopp22_amd import cabi

    return cabi.load()


# ---- 1. degrees ---------------------------------------------------------------------------------------------------------------------
DEGREE_n = [1, 31, 32, 33, 127, 128, 129, 1000, 4097]


def _check_degrees(adj, src, dst, n, what):
    """adj, adj.T: degrees() and mean_scale() of both views against the model, through to_old (the identity when not reordered)."""
    out_deg, in_deg = degrees(src, dst, n)
    for a, want in ((adj, out_deg), (adj.T, in_deg)):
        d, s = a.degrees(), a.mean_scale()
        assert str(d.dtype) == "torch.int32" and str(s.dtype) == "torch.float32" and d.shape == (n,) and s.shape == (n,), what
        np.testing.assert_array_equal(adj.to_old(d).cpu().numpy(), want, err_msg=f"{what} transposed={a.transposed}")
        assert_floats_identical(adj.to_old(s).cpu().numpy(), mean_scale(want), f"{what} scale transposed={a.transposed}")
    assert adj.T.degrees() is adj.T.degrees() and adj._degree_tensors() is adj.T._degree_tensors()   # one call, one cache


@pytest.mark.parametrize("n", DEGREE_n)
def test_degrees_equal_the_model(qgtc, n):
    import torch

    rng = np.random.default_rng(100 + n)
    src, dst = random_edges(rng, n, 6 * n + 5)
    dsrc, ddst = _dev(torch, src), _dev(torch, dst)
    _check_degrees(qgtc.pack_edges_tiled(dsrc, ddst, n), src, dst, n, "plain")
    re = qgtc.pack_edges_tiled(dsrc, ddst, n, reorder=True)
    assert re.perm is not None
    _check_degrees(re, src, dst, n, "reordered")
    empty = qgtc.pack_edges_tiled(_dev(torch, NO_EDGES[0]), _dev(torch, NO_EDGES[1]), n)
    assert empty.n_tiles == 0
    _check_degrees(empty, NO_EDGES[0], NO_EDGES[1], n, "no edges")


def test_degrees_at_the_largest_n(qgtc):
    """n = 2^23, the graph of test_tiled_variants_gpu.test_the_largest_n: corners, the last row block and the last k-quad."""
    import torch

    n = 1 << 23
    rng = np.random.default_rng(23)
    corner = np.array([[0, 0], [0, n - 1], [n - 1, 0], [n - 1, n - 1], [n - 1, n - 1], [n - 1, n - 1],
                       [n - 2, n - 3], [n - 2, n - 3], [n - 32, n - 128], [n - 31, 5], [127, n - 129]], dtype=np.int64)
    last = np.stack([rng.integers(n - 32, n, 300), rng.integers(n - 128, n, 300)], axis=1)
    spread = rng.integers(0, n, size=(20000, 2))
    e = np.concatenate([corner, last, spread, spread[:500], spread[:100]])
    src, dst = np.ascontiguousarray(e[:, 0]), np.ascontiguousarray(e[:, 1])
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    _check_degrees(adj, src, dst, n, "n = 2^23")
    assert int(adj.degrees()[n - 1]) >= 2 and int(adj.T.degrees()[n - 1]) >= 2      # (n-1, 0) / (0, n-1) and the 3-fold (n-1, n-1)


@pytest.mark.parametrize("n,edges", [(129, True), (4097, True), (300, False)])
def test_degrees_through_the_c_abi(qgtc, lib, n, edges):
    """Each allowed NULL combination: the given outputs are written in full (pre-filled with 0xA5), the canaries behind them stay."""
    import torch

    src, dst = random_edges(np.random.default_rng(n), n, 6 * n + 5) if edges else NO_EDGES
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    assert (adj.n_tiles > 0) == edges
    out_deg, in_deg = degrees(src, dst, n)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    combos = [(1, 0, 0, 0), (1, 0, 1, 0), (0, 1, 0, 0), (0, 1, 0, 1), (1, 1, 1, 1)]   # out_deg, in_deg, out_inv, in_inv
    for combo in combos:
        bufs = [torch.full((n + CANARY,), POISON_BITS, dtype=torch.int32, device="cuda") if on else None for on in combo]
        rc = lib.qgtc_tiled_degrees(_ptr(adj.row_ptr), _ptr(adj.kquad), _ptr(adj.tiles), adj.n_tiles, n,
                                    *[b.data_ptr() if b is not None else None for b in bufs], st)
        assert rc == 0, (combo, rc)
        for k, (b, want) in enumerate(zip(bufs, (out_deg, in_deg, mean_scale(out_deg), mean_scale(in_deg)))):
            if b is None:
                continue
            got = b.cpu().numpy()
            assert (got[n:].view(np.uint32) == np.uint32(0xA5A5A5A5)).all(), (combo, k, "canaries")
            if k < 2:
                np.testing.assert_array_equal(got[:n], want, err_msg=f"{combo} output {k}")
            else:
                assert_floats_identical(got[:n].view(np.float32), want, f"{combo} output {k}")


# ---- 2. the sweep: every variant, both directions, both outputs, three scales -----------------------------------------------------
# the sweep of the variants file (N over every variant boundary; graphs from n = 129 up have an empty row block), and two adjacencies
# without a tile, where every sum is 0 and the special scales give 0 * inf and 0 * NaN
SCALED_SWEEP = [(n, N, w, ob, True) for n, N, w, ob in SWEEP] + [(300, 24, 4, 4, False), (33, 130, 1, 2, False)]


@pytest.mark.parametrize("n,N,w,ob,edges", SCALED_SWEEP, ids=[f"n{n}-N{N}-w{w}-ob{ob}{'' if e else '-notiles'}" for n, N, w, ob, e in SCALED_SWEEP])
def test_every_variant_scaled_equals_the_model(qgtc, oracle, n, N, w, ob, edges):
    import torch

    rng = np.random.default_rng(7 * n + N)
    src, dst = random_edges(rng, n, 6 * n + 5) if edges else NO_EDGES
    Xq = rng.integers(0, 2 ** w, size=(n, N))
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    assert (adj.n_tiles > 0) == edges
    X = _bits_of(qgtc, torch, Xq, w)
    degs = degrees(src, dst, n)
    for a, transposed in ((adj, False), (adj.T, True)):
        C = aggregate(src, dst, n, Xq, transposed)
        if not transposed and edges and n >= 96:
            assert not C[32:64].any()              # the empty row block
        for kind, scale in _scales(rng, n, degs[1 if transposed else 0]).items():
            y = scaled(C, scale)
            if kind == "special" and n >= 8 and (not edges or n >= 96):
                assert np.isnan(y).any()           # 0 * inf, 0 * NaN rows occur
            what = f"{'adj.T' if transposed else 'adj'} R={variant(N, transposed)} scale={kind}"
            s = _dev(torch, scale)
            assert_floats_identical(qgtc.tiledMM2Int(a, X, N, w, s).cpu().numpy(), y, what)
            np.testing.assert_array_equal(to_np_u32(qgtc.tiledMM2Bit(a, X, N, w, ob, s)), expected_bits_scaled(oracle, y, ob), err_msg=what)


# ---- 3. poisoned outputs through the C-ABI ------------------------------------------------------------------------------------------
POISON = [(129, 16, 3, 5, True), (4097, 24, 2, 8, True), (33, 40, 8, 32, True), (1001, 200, 5, 3, True),
          (300, 24, 4, 4, False), (1, 130, 1, 2, False)]


@pytest.mark.parametrize("n,N,w,ob,edges", POISON)
def test_poisoned_outputs_through_the_c_abi(qgtc, oracle, lib, n, N, w, ob, edges):
    """Every word below the required size is written, nothing past it, with and without tiles (the scale: random positive floats)."""
    import torch

    rng = np.random.default_rng(n + N)
    src, dst = random_edges(rng, n, 6 * n + 5) if edges else NO_EDGES
    Xq = rng.integers(0, 2 ** w, size=(n, N))
    scale = rng.uniform(2.0 ** -10, 4.0, n).astype(np.float32)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    assert (adj.n_tiles > 0) == edges
    t = adj.T
    X, s = _bits_of(qgtc, torch, Xq, w), _dev(torch, scale)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    T, words, elems = adj.n_tiles, lib.qgtc_rows_words(n, N, ob), n * N
    fwd = (_ptr(adj.row_ptr), _ptr(adj.kquad), _ptr(adj.tiles), T, n, X.data_ptr(), X.numel(), N, w)
    tr = (_ptr(t.col_ptr), _ptr(t.col_tile), _ptr(t.col_rb), _ptr(adj.tiles), T, n, X.data_ptr(), X.numel(), N, w)
    for transposed, head in ((False, fwd), (True, tr)):
        y = scaled(aggregate(src, dst, n, Xq, transposed), scale)
        want = expected_bits_scaled(oracle, y, ob)
        assert want.size == words
        out = torch.full((words + CANARY,), POISON_BITS, dtype=torch.int32, device="cuda")
        call = lib.qgtc_tiledmm2bit_t_scaled if transposed else lib.qgtc_tiledmm2bit_scaled
        assert call(*head, ob, s.data_ptr(), out.data_ptr(), words, st) == 0
        got = to_np_u32(out)
        np.testing.assert_array_equal(got[:words], want, err_msg=f"bits transposed={transposed}")
        assert (got[words:] == np.uint32(0xA5A5A5A5)).all(), f"bits canaries transposed={transposed}"
        outf = torch.full((elems + CANARY,), float("nan"), dtype=torch.float32, device="cuda")
        call = lib.qgtc_tiledmm2int_t_scaled if transposed else lib.qgtc_tiledmm2int_scaled
        assert call(*head, s.data_ptr(), outf.data_ptr(), elems, st) == 0
        gotf = outf.cpu().numpy()
        assert not np.isnan(y).any()
        assert_floats_identical(gotf[:elems].reshape(n, N), y, f"floats transposed={transposed}")
        assert (gotf[elems:].view(np.uint32) == NAN_WORD).all(), f"float canaries transposed={transposed}"


# ---- 4. the defining identity, and a scale of ones ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n,N,w,ob", [SWEEP[5], SWEEP[9], SWEEP[16]], ids=lambda v: str(v))
def test_bits_are_val2bit_of_the_scaled_floats(qgtc, n, N, w, ob):
    """tiledMM2Bit(..., row_scale=s) == val2bit(tiledMM2Int(..., row_scale=s), ob, False, False), word for word, on the device."""
    import torch

    rng = np.random.default_rng(n * N)
    src, dst = random_edges(rng, n, 6 * n + 5)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    X = _bits_of(qgtc, torch, rng.integers(0, 2 ** w, size=(n, N)), w)
    for a in (adj, adj.T):
        for kind, scale in _scales(rng, n, a.degrees().cpu().numpy()).items():
            s = _dev(torch, scale)
            bits = qgtc.tiledMM2Bit(a, X, N, w, ob, s)
            assert torch.equal(bits, qgtc.val2bit(qgtc.tiledMM2Int(a, X, N, w, s), ob, False, False)), (a.transposed, kind)


@pytest.mark.parametrize("ob", [1, 2, 3, 8, 16, 23, 30])
def test_a_scale_of_ones_gives_the_unscaled_output(qgtc, ob):
    import torch

    n, N, w = 1000, 40, 8
    rng = np.random.default_rng(ob)
    src, dst = random_edges(rng, n, 6 * n + 5)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    X = _bits_of(qgtc, torch, rng.integers(0, 2 ** w, size=(n, N)), w)
    ones = torch.ones(n, dtype=torch.float32, device="cuda")
    for a in (adj, adj.T):
        assert torch.equal(qgtc.tiledMM2Bit(a, X, N, w, ob, ones), qgtc.tiledMM2Bit(a, X, N, w, ob)), a.transposed
        assert torch.equal(qgtc.tiledMM2Int(a, X, N, w, ones).view(torch.int32), qgtc.tiledMM2Int(a, X, N, w).view(torch.int32)), a.transposed


# ---- 5. hub sums at the float32 integer edge ----------------------------------------------------------------------------------------
def test_hub_sums_at_the_float_edge(qgtc, oracle):
    """Hub rows and hub columns summing to exactly 2^24 - 1, 2^24 + 1, 2^24 + 3 and 2^25 + 1 (built as
    test_tiled_variants_gpu.test_requant_at_the_float_compare_edge builds them: nodes below 131 586 carry 255, the rest 1), scaled by 1,
    0.5, 2^-20 and the mean scale: the int -> float conversion rounds to even (2^24 + 1 -> 2^24, 2^24 + 3 -> 2^24 + 4), and the
    quantiser rounds the scaled value's ties."""
    import torch

    n, N, w, big = 140000, 16, 8, 131586
    targets = [(65793, 0), (65793, 2), (65793, 4), (131586, 3)]
    hub_rows, hub_cols = [131600, 135000, 138000, n - 1], [131601, 135001, 138001, n - 10]
    rng = np.random.default_rng(24)
    src, dst = [], []
    for (a, b), h_r, h_c in zip(targets, hub_rows, hub_cols):
        nb = np.concatenate([np.arange(a), big + np.arange(b)]).astype(np.int64)
        src += [np.full(nb.size, h_r, np.int64), nb]
        dst += [nb, np.full(nb.size, h_c, np.int64)]
    s, d = rng.integers(0, n, 2 * n), rng.integers(0, n, 2 * n)
    keep = ~np.isin(s, hub_rows) & ~np.isin(d, hub_cols)
    src, dst = np.concatenate(src + [s[keep]]), np.concatenate(dst + [d[keep]])
    Xq = np.where(np.arange(n) < big, 255, 1)[:, None].repeat(N, axis=1)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    X = _bits_of(qgtc, torch, Xq, w)
    sums = [255 * a + b for a, b in targets]
    assert sums == [2 ** 24 - 1, 2 ** 24 + 1, 2 ** 24 + 3, 2 ** 25 + 1]
    degs = degrees(src, dst, n)
    for a, transposed, hubs in ((adj, False, hub_rows), (adj.T, True, hub_cols)):
        C = aggregate(src, dst, n, Xq, transposed)
        assert (C[hubs] == np.array(sums)[:, None]).all()
        deg = degs[1 if transposed else 0]
        assert deg[hubs].tolist() == [a_ + b_ for a_, b_ in targets]
        for name, scale in (("1", np.ones(n, np.float32)), ("0.5", np.full(n, 0.5, np.float32)),
                            ("2^-20", np.full(n, 2.0 ** -20, np.float32)), ("mean", mean_scale(deg))):
            y = scaled(C, scale)
            if name == "1":
                assert y[hubs, 0].tolist() == [2.0 ** 24 - 1, 2.0 ** 24, 2.0 ** 24 + 4, 2.0 ** 25]
            dscale = _dev(torch, scale)
            assert_floats_identical(qgtc.tiledMM2Int(a, X, N, w, dscale).cpu().numpy(), y, f"transposed={transposed} scale={name}")
            for ob in (8, 23, 24, 25, 32):
                np.testing.assert_array_equal(to_np_u32(qgtc.tiledMM2Bit(a, X, N, w, ob, dscale)), expected_bits_scaled(oracle, y, ob),
                                              err_msg=f"transposed={transposed} scale={name} ob={ob}")


# ---- 6. exact ties ---------------------------------------------------------------------------------------------------------------
def test_exact_half_ties_round_to_even(qgtc, oracle):
    """Rows of degree 2 and 4 in both directions (node u points at u + 1, u + 2, and every even node also at u + 4, u + 6, so even nodes
    have out- and in-degree 4, odd nodes 2): a mean of integers over 2 or 4 terms has fraction exactly one half whenever the sum is odd
    (degree 2) or 2 mod 4 (degree 4). At least 2 % of the outputs must be such ties below the clamp, so the quantiser's rounding mode
    decides them."""
    import torch

    n, N, w = 2000, 40, 3
    u = np.arange(n, dtype=np.int64)
    src = np.concatenate([u, u, u[::2], u[::2]])
    dst = np.concatenate([(u + 1) % n, (u + 2) % n, (u[::2] + 4) % n, (u[::2] + 6) % n])
    rng = np.random.default_rng(6)
    Xq = rng.integers(0, 2 ** w, size=(n, N))
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    X = _bits_of(qgtc, torch, Xq, w)
    degs = degrees(src, dst, n)
    for a, transposed in ((adj, False), (adj.T, True)):
        deg = degs[1 if transposed else 0]
        assert (deg[::2] == 4).all() and (deg[1::2] == 2).all()
        y = scaled(aggregate(src, dst, n, Xq, transposed), mean_scale(deg))
        ties = (y - np.floor(y) == np.float32(0.5)) & (y < 2 ** w)
        assert ties.mean() >= 0.02, ties.mean()
        q = oracle.quantize(y, w)
        assert (q[ties] % 2 == 0).all()            # half to even, and both neighbours occur
        assert (q[ties] > y[ties]).any() and (q[ties] < y[ties]).any()
        s = a.mean_scale()
        assert_floats_identical(s.cpu().numpy(), mean_scale(deg))
        assert_floats_identical(qgtc.tiledMM2Int(a, X, N, w, s).cpu().numpy(), y, f"transposed={transposed}")
        np.testing.assert_array_equal(to_np_u32(qgtc.tiledMM2Bit(a, X, N, w, w, s)), expected_bits_scaled(oracle, y, w),
                                      err_msg=f"transposed={transposed}")


# ---- 7. the module ------------------------------------------------------------------------------------------------------------------
def _model_forward(oracle, m, src, dst, n, X, transposed):
    """GCNConv_Qnt(aggr="mean") layer by layer: each X . W from the oracle's bitmm2bit(col=True) on the previous layer's packed
    activations, unpacked; each aggregate from the scaled model."""
    f_in, hid, f_out, a, w = m.input_dim, m.hidden_dim, m.output_dim, m.act_bit, m.w_bit
    W_in = oracle.val2bit(m.W_in.detach().cpu().numpy(), w, True)
    W_out = oracle.val2bit(m.W_out.detach().cpu().numpy(), w, True)
    scale = mean_scale(degrees(src, dst, n)[1 if transposed else 0])
    bit_X = oracle.val2bit(X, a)
    t = oracle.bit2val(oracle.bitmm2bit(bit_X, W_in, n, f_in, hid, a, w, a, col=True), a, n, hid, col_major=True)
    y = scaled(aggregate(src, dst, n, t, transposed), scale)
    bit_h = oracle.pack(oracle.quantize(y, a), a)
    t = oracle.bit2val(oracle.bitmm2bit(bit_h, W_out, n, hid, f_out, a, w, a, col=True), a, n, f_out, col_major=True)
    return scaled(aggregate(src, dst, n, t, transposed), scale)


@pytest.mark.parametrize("n", [200, 1213])
def test_module_mean_equals_the_model(qgtc, oracle, n):
    import torch

    from qgtc_ppopp22_amd.conv import GCNConv_Qnt

    torch.manual_seed(0)
    rng = np.random.default_rng(n)
    src, dst = random_edges(rng, n, 8 * n)
    dsrc, ddst = _dev(torch, src), _dev(torch, dst)
    m = GCNConv_Qnt(48, 64, 10, w_bit=2, act_bit=3, aggr="mean").cuda()
    with torch.no_grad():                          # sparse weights and features: X . W stays below requant's clamp, so the layers differ
        m.W_in.mul_((torch.rand_like(m.W_in) < 0.08).float())
        m.W_out.mul_((torch.rand_like(m.W_out) < 0.08).float())
    X = (torch.randn(n, 48, device="cuda") * 2 + 2) * (torch.rand(n, 48, device="cuda") < 0.15).float()
    adj, re = qgtc.pack_edges_tiled(dsrc, ddst, n), qgtc.pack_edges_tiled(dsrc, ddst, n, reorder=True)
    for transposed in (False, True):
        want = _model_forward(oracle, m, src, dst, n, X.cpu().numpy(), transposed)
        got = m(adj.T if transposed else adj, X)
        assert got.dtype == torch.float32 and got.shape == (n, 10)
        assert_floats_identical(got.cpu().numpy(), want, f"transposed={transposed}")
        assert len(np.unique(want)) > 16           # the case tells the layers apart: not the constant a saturated chain gives
        got_re = m(re.T if transposed else re, X)
        assert torch.equal(got_re.view(torch.int32), got.view(torch.int32)), f"reordered, transposed={transposed}"


def test_module_sum_is_unchanged_and_refusals(qgtc):
    import torch

    from qgtc_ppopp22_amd.conv import GCNConv_Qnt

    n = 400
    torch.manual_seed(0)
    src, dst = random_edges(np.random.default_rng(n), n, 8 * n)
    dsrc, ddst = _dev(torch, src), _dev(torch, dst)
    X = torch.randn(n, 48, device="cuda")
    adj = qgtc.pack_edges_tiled(dsrc, ddst, n)
    default = GCNConv_Qnt(48, 64, 10, w_bit=2, act_bit=3).cuda()
    assert default.aggr == "sum"
    explicit = GCNConv_Qnt(48, 64, 10, w_bit=2, act_bit=3, aggr="sum").cuda()
    explicit.load_state_dict(default.state_dict())
    want = default((dsrc, ddst, n), X)             # the edge-list route: no tiled kernel involved
    assert torch.equal(default(adj, X), want) and torch.equal(explicit(adj, X), want) and torch.equal(explicit((dsrc, ddst, n), X), want)
    with pytest.raises(ValueError):
        GCNConv_Qnt(48, 64, 10, aggr="max")
    mean = GCNConv_Qnt(48, 64, 10, w_bit=2, act_bit=3, aggr="mean").cuda()
    with pytest.raises(NotImplementedError, match="pack_edges_tiled"):
        mean((dsrc, ddst, n), X)
    with pytest.raises(NotImplementedError, match="pack_edges_tiled"):
        mean(torch.zeros(n, n, device="cuda"), X)


# ---- 8. Python argument refusals ----------------------------------------------------------------------------------------------------
def test_row_scale_refusals(qgtc):
    import torch

    n, N, w = 100, 8, 2
    src, dst = random_edges(np.random.default_rng(8), n, 6 * n)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    X = _bits_of(qgtc, torch, np.ones((n, N)), w)
    good = torch.ones(n, dtype=torch.float32, device="cuda")
    bad = [(TypeError, good.double()), (TypeError, good.to(torch.int32)), (TypeError, [1.0] * n), (TypeError, 1.0),
           (ValueError, torch.ones(n - 1, dtype=torch.float32, device="cuda")), (ValueError, torch.ones(n + 1, dtype=torch.float32, device="cuda")),
           (ValueError, torch.ones(n, 1, dtype=torch.float32, device="cuda")), (ValueError, good.cpu()),
           (ValueError, torch.ones(2 * n, dtype=torch.float32, device="cuda")[::2])]
    for a in (adj, adj.T):
        for exc, s in bad:
            with pytest.raises(exc):
                qgtc.tiledMM2Int(a, X, N, w, s)
            with pytest.raises(exc):
                qgtc.tiledMM2Bit(a, X, N, w, 2, row_scale=s)
        assert qgtc.tiledMM2Int(a, X, N, w, row_scale=good).shape == (n, N)
