"""Every template variant of the tiled products (k_tiled_mm for adj, k_tiled_mm_t for adj.T; tests/tiled_model.py's `variant` states
which N picks which) against the exact edge-list model of tests/tiled_model.py, word for word and value for value: a sweep of N over
every variant boundary through both entries, poisoned outputs through the C-ABI (every word below the required size written, nothing
past it), requant's float compare at sums of 2^24 +- 1 and 2^25 + 1, and the domain's upper end n = 2^23."""
import ctypes

import numpy as np
import pytest

from helpers import to_np_u32
from qgtc_ppopp22_amd.shapes import P8, S128
from tiled_model import (FORWARD_VARIANTS, TRANSPOSED_VARIANTS, aggregate, expected_bits, expected_floats, np_colindex, np_tiled,
                         random_edges, requant, variant)

pytestmark = pytest.mark.gpu


# N over every variant boundary of both kernels (16 / 32 / 64 and the 128-column chunks); n, bit2 and ob rotate alongside
SWEEP_N = [1, 15, 16, 17, 24, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 383]
SWEEP_n = [1, 31, 33, 127, 129, 1000, 4097]
SWEEP_OB = [1, 2, 3, 5, 8, 16, 23, 32]
SWEEP = [(SWEEP_n[i % 7], N, i % 8 + 1, SWEEP_OB[3 * i % 8]) for i, N in enumerate(SWEEP_N)]


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits_of(qgtc, torch, Xq, w):
    """X in the cols layout, from the quantised features."""
    return qgtc.val2bit(torch.from_numpy(np.ascontiguousarray(Xq, dtype=np.float32)).cuda(), w, True, False)


def test_the_sweep_hits_every_variant():
    """Each sweep case runs both directions through both entries (bits and float), so every variant of both kernels meets both
    output kinds, at a ragged N and at its full width."""
    for transposed, variants in ((False, FORWARD_VARIANTS), (True, TRANSPOSED_VARIANTS)):
        hit = {}
        for _, N, _, _ in SWEEP:
            hit.setdefault(variant(N, transposed), set()).add(N)
        assert sorted(hit) == sorted(variants)
        assert all(len(Ns) >= 2 for Ns in hit.values()), hit
    assert any(N > 256 for N in SWEEP_N)   # three 128-column chunks of the widest variants


@pytest.mark.parametrize("n,N,w,ob", SWEEP, ids=[f"n{n}-N{N}-w{w}-ob{ob}" for n, N, w, ob in SWEEP])
def test_every_variant_equals_the_edge_list_model(qgtc, oracle, n, N, w, ob):
    import torch

    rng = np.random.default_rng(7 * n + N)
    src, dst = random_edges(rng, n, 6 * n + 5)
    Xq = rng.integers(0, 2 ** w, size=(n, N))
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    X = _bits_of(qgtc, torch, Xq, w)
    for a, transposed in ((adj, False), (adj.T, True)):
        C = aggregate(src, dst, n, Xq, transposed)
        if transposed and n >= 512:
            assert not C[128:256].any()            # the empty k-quad: zero rows of the transposed product
        if not transposed and n >= 96:
            assert not C[32:64].any()              # the empty row block
        what = f"{'adj.T' if transposed else 'adj'} R={variant(N, transposed)}"
        np.testing.assert_array_equal(to_np_u32(qgtc.tiledMM2Bit(a, X, N, w, ob)), expected_bits(oracle, C, ob), err_msg=what)
        np.testing.assert_array_equal(qgtc.tiledMM2Int(a, X, N, w).cpu().numpy(), expected_floats(C), err_msg=what)


# ---- poisoned outputs through the C-ABI ---------------------------------------------------------------------------------------------
CANARY = 64
POISON_BITS = -0x5A5A5A5B                          # 0xA5A5A5A5 as int32
NAN_WORD = 0x7FC00000                              # the float NaN torch.full writes


@pytest.fixture(scope="module")
def lib():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    from qgtc_ppopp22_amd import cabi

    return cabi.load()


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def _colindex(torch, lib, adj, st):
    """The column index straight from qgtc_tiled_colindex into caller-owned buffers."""
    n, T = adj.n, adj.n_tiles
    col_ptr = torch.empty(S128(n) + 1, dtype=torch.int64, device="cuda")
    col_tile = torch.empty(T, dtype=torch.int64, device="cuda") if T else None
    col_rb = torch.empty(T, dtype=torch.int32, device="cuda") if T else None
    work, ww = None, 0
    if T:
        ww = lib.qgtc_tiled_colindex_work_words(T)
        work = torch.empty(ww, dtype=torch.int32, device="cuda")
        assert work.data_ptr() % 256 == 0
    rc = lib.qgtc_tiled_colindex(_ptr(adj.row_ptr), _ptr(adj.kquad), T, n, col_ptr.data_ptr(), _ptr(col_tile), _ptr(col_rb),
                                 _ptr(work), ww, st)
    assert rc == 0, rc
    return col_ptr, col_tile, col_rb


# (n, N, w, ob, edges): one N per variant of both kernels (n not a multiple of 8: padding rows; N not a multiple of 128: padding
# words), and adjacencies without a tile
POISON = [(129, 16, 3, 5, True), (4097, 24, 2, 8, True), (33, 40, 8, 32, True), (1001, 200, 5, 3, True),
          (300, 24, 4, 4, False), (1, 130, 1, 2, False)]


@pytest.mark.parametrize("n,N,w,ob,edges", POISON)
def test_poisoned_outputs_through_the_c_abi(qgtc, oracle, lib, n, N, w, ob, edges):
    import torch

    rng = np.random.default_rng(n + N)
    src, dst = random_edges(rng, n, 6 * n + 5) if edges else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    Xq = rng.integers(0, 2 ** w, size=(n, N))
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    assert (adj.n_tiles > 0) == edges
    X = _bits_of(qgtc, torch, Xq, w)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    col_ptr, col_tile, col_rb = _colindex(torch, lib, adj, st)
    want_idx = np_colindex(adj.row_ptr.cpu().numpy(), adj.kquad.cpu().numpy(), n)
    np.testing.assert_array_equal(col_ptr.cpu().numpy(), want_idx[0])
    if edges:
        np.testing.assert_array_equal(col_tile.cpu().numpy(), want_idx[1])
        np.testing.assert_array_equal(col_rb.cpu().numpy(), want_idx[2])
    T, words, elems = adj.n_tiles, lib.qgtc_rows_words(n, N, ob), n * N
    fwd = (_ptr(adj.row_ptr), _ptr(adj.kquad), _ptr(adj.tiles), T, n, X.data_ptr(), X.numel(), N, w)
    tr = (_ptr(col_ptr), _ptr(col_tile), _ptr(col_rb), _ptr(adj.tiles), T, n, X.data_ptr(), X.numel(), N, w)
    for transposed, head in ((False, fwd), (True, tr)):
        C = aggregate(src, dst, n, Xq, transposed)
        want = expected_bits(oracle, C, ob)
        assert want.size == words
        out = torch.full((words + CANARY,), POISON_BITS, dtype=torch.int32, device="cuda")
        call = lib.qgtc_tiledmm2bit_t if transposed else lib.qgtc_tiledmm2bit
        assert call(*head, ob, out.data_ptr(), words, st) == 0
        got = to_np_u32(out)
        np.testing.assert_array_equal(got[:words], want, err_msg=f"bits transposed={transposed}")
        assert (got[words:] == np.uint32(0xA5A5A5A5)).all(), f"bits canaries transposed={transposed}"
        outf = torch.full((elems + CANARY,), float("nan"), dtype=torch.float32, device="cuda")
        call = lib.qgtc_tiledmm2int_t if transposed else lib.qgtc_tiledmm2int
        assert call(*head, outf.data_ptr(), elems, st) == 0
        gotf = outf.cpu().numpy()
        np.testing.assert_array_equal(gotf[:elems].reshape(n, N), expected_floats(C), err_msg=f"floats transposed={transposed}")
        assert (gotf[elems:].view(np.uint32) == NAN_WORD).all(), f"float canaries transposed={transposed}"


# ---- requant's float compare ---------------------------------------------------------------------------------------------------
def test_requant_at_the_float_compare_edge(qgtc, oracle):
    """Hub rows (out-neighbour sums) and hub columns (in-neighbour sums) of exactly 2^24 - 1, 2^24, 2^24 + 1 and 2^25 + 1: nodes below
    131 586 carry 255, the rest 1, so a hub with a nodes of 255 and b of 1 sums to 255 a + b. At ob >= 24 requant compares in float32,
    where 2^24 + 1 and 2^25 + 1 round down."""
    import torch

    n, N, w, big = 140000, 16, 8, 131586
    targets = [(65793, 0), (65793, 1), (65793, 2), (131586, 3)]          # 2^24 - 1, 2^24, 2^24 + 1, 2^25 + 1
    hub_rows, hub_cols = [131600, 135000, 138000, n - 1], [131601, 135001, 138001, n - 10]   # in no hub's neighbour set
    rng = np.random.default_rng(24)
    src, dst = [], []
    for (a, b), h_r, h_c in zip(targets, hub_rows, hub_cols):
        nb = np.concatenate([np.arange(a), big + np.arange(b)]).astype(np.int64)
        src += [np.full(nb.size, h_r, np.int64), nb]
        dst += [nb, np.full(nb.size, h_c, np.int64)]
    s, d = rng.integers(0, n, 2 * n), rng.integers(0, n, 2 * n)
    keep = ~np.isin(s, hub_rows) & ~np.isin(d, hub_cols)                # the hubs' sums stay exact
    src, dst = np.concatenate(src + [s[keep]]), np.concatenate(dst + [d[keep]])
    Xq = np.where(np.arange(n) < big, 255, 1)[:, None].repeat(N, axis=1)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    X = _bits_of(qgtc, torch, Xq, w)
    sums = [255 * a + b for a, b in targets]
    assert sums == [2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 25 + 1]
    for a, transposed, hubs in ((adj, False, hub_rows), (adj.T, True, hub_cols)):
        C = aggregate(src, dst, n, Xq, transposed)
        assert (C[hubs] == np.array(sums)[:, None]).all()
        np.testing.assert_array_equal(qgtc.tiledMM2Int(a, X, N, w).cpu().numpy(), expected_floats(C))
        for ob in (23, 24, 25, 31, 32):
            got = to_np_u32(qgtc.tiledMM2Bit(a, X, N, w, ob))
            np.testing.assert_array_equal(got, expected_bits(oracle, C, ob), err_msg=f"transposed={transposed} ob={ob}")
            # the hubs decode to the oracle's requant of their sums
            planes = got.reshape(ob, P8(n), S128(N) * 4)[:, hubs, 0] >> np.uint32(31)
            dec = (planes.astype(np.int64) << np.arange(ob)[:, None]).sum(axis=0)
            assert dec.tolist() == [int(requant(oracle, s, ob)) & (2 ** ob - 1) for s in sums], (transposed, ob)


# ---- the domain's upper end ------------------------------------------------------------------------------------------------------
def _features_2_23(v, j):
    """Quantised 2-bit features of node v, column j: the same formula on the device and the host."""
    return (v * 7919 + j * 104729 + (v >> 9)) % 4


def test_the_largest_n(qgtc, oracle):
    """n = 2^23, where the 47-bit cell key and the column index run at their limits: a sparse graph touching nodes 0 and 2^23 - 1, the
    last row block and the last k-quad. The format and the index against the model; the products at N = 16, bit2 = 2 on the device:
    the touched rows equal the model on the touched nodes, every other row is zero."""
    import torch

    n, N, w, ob = 1 << 23, 16, 2, 3
    rng = np.random.default_rng(23)
    corner = np.array([[0, 0], [0, n - 1], [n - 1, 0], [n - 1, n - 1], [n - 1, n - 1], [n - 1, n - 1],   # (n-1, n-1) 3-fold: set
                       [n - 2, n - 3], [n - 2, n - 3], [n - 32, n - 128], [n - 31, 5], [127, n - 129]], dtype=np.int64)
    last = np.stack([rng.integers(n - 32, n, 300), rng.integers(n - 128, n, 300)], axis=1)                # last block, last k-quad
    spread = rng.integers(0, n, size=(20000, 2))
    e = np.concatenate([corner, last, spread, spread[:500], spread[:100]])                             # multiplicities 2 and 3
    src, dst = np.ascontiguousarray(e[:, 0]), np.ascontiguousarray(e[:, 1])
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    row_ptr, kquad, tiles = np_tiled(src, dst, n)
    np.testing.assert_array_equal(adj.row_ptr.cpu().numpy(), row_ptr)
    np.testing.assert_array_equal(adj.kquad.cpu().numpy(), kquad)
    np.testing.assert_array_equal(adj.tiles.cpu().numpy().view(np.uint32), tiles)
    assert kquad[-1] == S128(n) - 1 and row_ptr[-2] < row_ptr[-1]                                       # the last tile is the corner
    col_ptr, col_tile, col_rb = np_colindex(row_ptr, kquad, n)
    t = adj.T
    np.testing.assert_array_equal(t.col_ptr.cpu().numpy(), col_ptr)
    np.testing.assert_array_equal(t.col_tile.cpu().numpy(), col_tile)
    np.testing.assert_array_equal(t.col_rb.cpu().numpy(), col_rb)

    # the model on the touched nodes only (a relabelling keeps every cell's multiplicity)
    nodes = np.unique(np.concatenate([src, dst]))
    m = nodes.size
    Xq_c = _features_2_23(nodes[:, None], np.arange(N)[None, :])
    v = torch.arange(n, device="cuda", dtype=torch.int64)[:, None]
    j = torch.arange(N, device="cuda", dtype=torch.int64)[None, :]
    X = qgtc.val2bit(_features_2_23(v, j).to(torch.float32), w, True, False)
    del v, j
    rows = torch.from_numpy(nodes).cuda()
    for a, transposed in ((adj, False), (t, True)):
        C = aggregate(np.searchsorted(nodes, src), np.searchsorted(nodes, dst), m, Xq_c, transposed)
        f = qgtc.tiledMM2Int(a, X, N, w)
        np.testing.assert_array_equal(f[rows].cpu().numpy(), expected_floats(C), err_msg=f"floats transposed={transposed}")
        f[rows] = 0.0
        assert not f.any(), f"floats transposed={transposed}: a row without neighbours is not zero"
        del f
        b = qgtc.tiledMM2Bit(a, X, N, w, ob).view(ob, n, S128(N) * 4)
        want = expected_bits(oracle, C, ob).reshape(ob, P8(m), S128(N) * 4)[:, :m]
        np.testing.assert_array_equal(to_np_u32(b[:, rows]).reshape(want.shape), want, err_msg=f"bits transposed={transposed}")
        b[:, rows] = 0
        assert not b.any(), f"bits transposed={transposed}: a row without neighbours is not zero"
        del b
