"""The transposed tiled adjacency (TiledAdjacency.T, QGTC.tiledMM2Bit / tiledMM2Int on it, GCNConv_Qnt with adj.T): the column index
element for element against a NumPy model, and the products word for word against the forward products on the adjacency packed from
the reversed edge list, the dense route under every engine and the C oracle; sums past 2^24, a reordered adjacency, the module and a
graph beyond the dense cap."""
import numpy as np
import pytest

from helpers import ENGINES, to_np_u32, use_engine
from qgtc_ppopp22_amd.shapes import P8, S128
from tiled_model import np_colindex, random_edges

pytestmark = pytest.mark.gpu

NS = [1, 31, 129, 1000, 4097, 70000]


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _features(torch, rng, n, N, w):
    return torch.from_numpy(rng.integers(0, 2 ** w, size=(n, N)).astype(np.float32)).cuda()


def _graph(n, seed=0):
    rng = np.random.default_rng(1000 + n + seed)
    return random_edges(rng, n, 6 * n + 5)


@pytest.mark.parametrize("n", NS)
def test_index_matches_the_numpy_model(qgtc, n):
    import torch

    src, dst = _graph(n)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    t = adj.T
    assert t.transposed and not adj.transposed and t.T is adj and adj.T is t
    assert t.row_ptr is adj.row_ptr and t.kquad is adj.kquad and t.tiles is adj.tiles
    col_ptr, col_tile, col_rb = np_colindex(adj.row_ptr.cpu().numpy(), adj.kquad.cpu().numpy(), n)
    np.testing.assert_array_equal(t.col_ptr.cpu().numpy(), col_ptr)
    np.testing.assert_array_equal(t.col_tile.cpu().numpy(), col_tile)
    np.testing.assert_array_equal(t.col_rb.cpu().numpy(), col_rb)
    assert t.col_ptr.dtype == torch.int64 and t.col_tile.dtype == torch.int64 and t.col_rb.dtype == torch.int32
    assert t.nbytes == adj.nbytes + 8 * col_ptr.size + 12 * col_tile.size
    assert t.max_block_tiles == (int(np.diff(col_ptr).max()) if col_ptr.size > 1 else 0)
    assert "transposed=True" in repr(t) and "transposed=False" in repr(adj)
    if n >= 384:
        assert col_ptr[1] == col_ptr[2]            # the empty column group
    if n <= 5000:                                  # to_rows is dense: a test aid for small n
        assert torch.equal(t.to_rows(), qgtc.pack_edges(_dev(torch, dst), _dev(torch, src), n, n, 1))


def test_index_of_an_empty_adjacency(qgtc):
    import torch

    adj = qgtc.pack_edges_tiled(_dev(torch, np.zeros(0, np.int64)), _dev(torch, np.zeros(0, np.int64)), 300)
    t = adj.T
    assert t.n_tiles == 0 and t.col_tile.numel() == 0 and t.col_rb.numel() == 0
    np.testing.assert_array_equal(t.col_ptr.cpu().numpy(), np.zeros(4, np.int64))
    X = qgtc.val2bit(torch.ones(300, 20, device="cuda"), 2, True, False)
    assert not qgtc.tiledMM2Bit(t, X, 20, 2, 3).any()
    assert not qgtc.tiledMM2Int(t, X, 20, 2).any()


# (n, N, w, ob): n over NS, N over {1, 7, 17, 64, 128, 129, 300} (every kernel variant), w over 1 .. 8, ob over {1, 2, 3, 8, 16, 32}
PRODUCTS = [
    (1, 1, 1, 1),
    (31, 7, 2, 2),
    (129, 64, 3, 3),
    (1000, 128, 4, 8),
    (4097, 129, 5, 32),
    (70000, 300, 6, 3),
    (1000, 1, 7, 1),
    (4097, 7, 8, 8),
    (129, 300, 8, 32),
    (70000, 64, 1, 2),
    (31, 129, 2, 32),
    (4097, 128, 1, 1),
    (4097, 17, 4, 16),
]


@pytest.mark.parametrize("n,N,w,ob", PRODUCTS)
def test_products_equal_the_reversed_pack(qgtc, n, N, w, ob):
    import torch

    src, dst = _graph(n, N + w + ob)
    dsrc, ddst = _dev(torch, src), _dev(torch, dst)
    adj = qgtc.pack_edges_tiled(dsrc, ddst, n)
    rev = qgtc.pack_edges_tiled(ddst, dsrc, n)
    X = qgtc.val2bit(_features(torch, np.random.default_rng(n + N), n, N, w), w, True, False)
    got_b = qgtc.tiledMM2Bit(adj.T, X, N, w, ob)
    got_f = qgtc.tiledMM2Int(adj.T, X, N, w)
    assert got_b.shape == (ob * P8(n), S128(N) * 4) and got_f.shape == (n, N) and got_f.dtype == torch.float32
    assert torch.equal(got_b, qgtc.tiledMM2Bit(rev, X, N, w, ob))
    assert torch.equal(got_f, qgtc.tiledMM2Int(rev, X, N, w))
    # the forward product is untouched by the transposed view
    assert torch.equal(qgtc.tiledMM2Int(adj, X, N, w), qgtc.tiledMM2Int(rev.T, X, N, w))


@pytest.mark.parametrize("n,N,w,ob", [(31, 7, 2, 2), (129, 64, 3, 3), (1000, 128, 4, 8), (4097, 300, 8, 32), (1000, 16, 1, 1)])
def test_products_equal_the_dense_route(qgtc, n, N, w, ob):
    import torch

    src, dst = _graph(n, 7)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    A_rev = qgtc.pack_edges(_dev(torch, dst), _dev(torch, src), n, n, 1)
    X = qgtc.val2bit(_features(torch, np.random.default_rng(n), n, N, w), w, True, False)
    got_b = qgtc.tiledMM2Bit(adj.T, X, N, w, ob)
    got_f = qgtc.tiledMM2Int(adj.T, X, N, w)
    for eng in ENGINES:
        with use_engine(qgtc, eng):
            assert torch.equal(got_b, qgtc.bitMM2Bit(A_rev, X, n, n, N, 1, w, ob)), eng
            assert torch.equal(got_f, qgtc.bitMM2Int(A_rev, X, n, n, N, 1, w, True)), eng
            assert torch.equal(qgtc.tiledMM2Bit(adj.T, X, N, w, ob), got_b)


@pytest.mark.parametrize("n,N,w,ob", [(40, 10, 2, 3), (300, 64, 4, 8), (161, 130, 8, 32)])
def test_products_equal_the_oracle(qgtc, oracle, n, N, w, ob):
    import torch

    rng = np.random.default_rng(n)
    src, dst = random_edges(rng, n, 5 * n)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    AtSum = np.zeros((n, n), dtype=np.float32)
    np.add.at(AtSum, (dst, src), 1.0)
    Xf = rng.integers(0, 2 ** w, size=(n, N)).astype(np.float32)
    oA, oX = oracle.val2bit(AtSum, 1), oracle.val2bit(Xf, w, True)
    X = qgtc.val2bit(torch.from_numpy(Xf).cuda(), w, True, False)
    np.testing.assert_array_equal(to_np_u32(qgtc.tiledMM2Bit(adj.T, X, N, w, ob)), oracle.bitmm2bit(oA, oX, n, n, N, 1, w, ob))
    np.testing.assert_array_equal(qgtc.tiledMM2Int(adj.T, X, N, w).cpu().numpy(), oracle.bitmm2int(oA, oX, n, n, N, 1, w, True))


def test_hub_column_sums_past_two_to_the_24(qgtc):
    import torch

    n, N, hub = 70000, 40, 12345
    rng = np.random.default_rng(5)
    dst = np.concatenate([np.full(n, hub, np.int64), rng.integers(0, n, size=3 * n, dtype=np.int64)])
    src = np.concatenate([np.arange(n, dtype=np.int64), rng.integers(0, n, size=3 * n, dtype=np.int64)])
    keep = dst != hub
    keep[:n] = True                                   # the hub column: every node points at it exactly once
    src, dst = src[keep], dst[keep]
    dsrc, ddst = _dev(torch, src), _dev(torch, dst)
    adj = qgtc.pack_edges_tiled(dsrc, ddst, n)
    X = qgtc.val2bit(torch.full((n, N), 255.0, device="cuda"), 8, True, False)
    f = qgtc.tiledMM2Int(adj.T, X, N, 8)
    assert (f[hub] == 17850000.0).all()
    b = qgtc.tiledMM2Bit(adj.T, X, N, 8, 32)
    words = to_np_u32(b).reshape(32, P8(n), S128(N) * 4)
    col0 = [(int(words[p, hub, 0]) >> 31) & 1 for p in range(32)]
    assert sum(v << p for p, v in enumerate(col0)) == 17850000
    A_rev = qgtc.pack_edges(ddst, dsrc, n, n, 1)
    assert torch.equal(f, qgtc.bitMM2Int(A_rev, X, n, n, N, 1, 8, True))
    assert torch.equal(b, qgtc.bitMM2Bit(A_rev, X, n, n, N, 1, 8, 32))


@pytest.mark.parametrize("n", [300, 4097])
def test_symmetric_graph(qgtc, n):
    import torch

    rng = np.random.default_rng(n)
    s, d = rng.integers(0, n, 4 * n), rng.integers(0, n, 4 * n)
    src, dst = np.concatenate([s, d]), np.concatenate([d, s])
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    for N, w, ob in ((16, 2, 3), (200, 4, 8)):
        X = qgtc.val2bit(_features(torch, rng, n, N, w), w, True, False)
        assert torch.equal(qgtc.tiledMM2Bit(adj.T, X, N, w, ob), qgtc.tiledMM2Bit(adj, X, N, w, ob))
        assert torch.equal(qgtc.tiledMM2Int(adj.T, X, N, w), qgtc.tiledMM2Int(adj, X, N, w))


@pytest.mark.parametrize("n", [1000, 4097])
def test_reordered_adjacency(qgtc, n):
    import torch

    src, dst = _graph(n, 3)
    dsrc, ddst = _dev(torch, src), _dev(torch, dst)
    plain = qgtc.pack_edges_tiled(dsrc, ddst, n)
    adj = qgtc.pack_edges_tiled(dsrc, ddst, n, reorder=True)
    t = adj.T
    assert t.perm is adj.perm and t.rank is adj.rank
    N, w = 48, 3
    Xf = _features(torch, np.random.default_rng(n), n, N, w)
    want = qgtc.tiledMM2Int(plain.T, qgtc.val2bit(Xf, w, True, False), N, w)
    got = t.to_old(qgtc.tiledMM2Int(t, qgtc.val2bit(t.to_new(Xf), w, True, False), N, w))
    assert torch.equal(got, want)
    want_b = qgtc.tiledMM2Bit(plain.T, qgtc.val2bit(Xf, w, True, False), N, w, 4)
    got_b = t.to_old_packed(qgtc.tiledMM2Bit(t, qgtc.val2bit(t.to_new(Xf), w, True, False), N, w, 4), 4)
    assert torch.equal(got_b, want_b)


@pytest.mark.parametrize("reorder", [False, True])
@pytest.mark.parametrize("n", [300, 4096])
def test_module_on_the_transpose_equals_the_reversed_edge_list(qgtc, n, reorder):
    import torch

    from qgtc_ppopp22_amd.conv import GCNConv_Qnt

    torch.manual_seed(0)
    rng = np.random.default_rng(n)
    src, dst = random_edges(rng, n, 8 * n)
    dsrc, ddst = _dev(torch, src), _dev(torch, dst)
    m = GCNConv_Qnt(48, 64, 10, w_bit=2, act_bit=3).cuda()
    X = torch.randn(n, 48, device="cuda")
    want = m((ddst, dsrc, n), X)
    got = m(qgtc.pack_edges_tiled(dsrc, ddst, n, reorder=reorder).T, X)
    assert got.dtype == torch.float32 and got.shape == (n, 10)
    assert torch.equal(got, want)


def test_beyond_the_dense_cap(qgtc):
    """A reddit-sized directed SBM (232 965 nodes, past the dense route's operand cap): the transposed products equal the forward
    products on the reverse-packed adjacency."""
    import torch

    from qgtc_ppopp22_amd.graph import make_sbm_graph

    g = make_sbm_graph("reddit-sized", 232965, 1500, 20.0, 8, seed=4)
    n = g.n_nodes
    dsrc, ddst = _dev(torch, g.src), _dev(torch, g.dst)
    adj = qgtc.pack_edges_tiled(dsrc, ddst, n)
    rev = qgtc.pack_edges_tiled(ddst, dsrc, n)
    rng = np.random.default_rng(8)
    for N, w, ob in ((64, 2, 4), (256, 1, 1)):
        X = qgtc.val2bit(_features(torch, rng, n, N, w), w, True, False)
        assert torch.equal(qgtc.tiledMM2Bit(adj.T, X, N, w, ob), qgtc.tiledMM2Bit(rev, X, N, w, ob))
        assert torch.equal(qgtc.tiledMM2Int(adj.T, X, N, w), qgtc.tiledMM2Int(rev, X, N, w))


def test_errors(qgtc):
    import torch

    n = 300
    src, dst = _graph(n)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    X = qgtc.val2bit(torch.ones(n, 20, device="cuda"), 2, True, False)
    short = X.view(-1)[: X.numel() - 4].contiguous()
    with pytest.raises(RuntimeError):
        qgtc.tiledMM2Int(adj.T, short, 20, 2)
    with pytest.raises(RuntimeError):
        qgtc.tiledMM2Bit(adj.T, X, 20, 9, 2)
    with pytest.raises(TypeError):
        qgtc.tiledMM2Bit((adj.T.col_ptr, adj.T.col_tile, adj.T.col_rb, adj.tiles), X, 20, 2, 2)
    with pytest.raises(TypeError):
        qgtc.tiledMM2Int(qgtc.pack_edges(_dev(torch, src), _dev(torch, dst), n, n, 1), X, 20, 2)
