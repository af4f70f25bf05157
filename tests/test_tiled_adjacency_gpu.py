"""The tile-compressed whole-graph adjacency (QGTC.pack_edges_tiled, QGTC.tiledMM2Bit / tiledMM2Int, GCNConv_Qnt with a
TiledAdjacency): the format against a NumPy model, the products word for word against the dense route on pack_edges' words
(under every engine) and the C oracle, sums past 2^24, a graph beyond the dense route's 4 GiB operand cap, and the module."""
import numpy as np
import pytest

from helpers import ENGINES, to_np_u32, use_engine
from qgtc_ppopp22_amd.shapes import P8, S128
from tiled_model import np_tiled

pytestmark = pytest.mark.gpu


def random_edges(rng, n, e, dup=True, self_loops=True, empty_block=True):
    """Random edges with duplicates of multiplicity 2, 3 and 4, self loops, a hub row and (n >= 96) an empty row block."""
    src = rng.integers(0, n, size=e, dtype=np.int64)
    dst = rng.integers(0, n, size=e, dtype=np.int64)
    if n > 2:
        src[: e // 8] = n // 2                     # a hub row
    if empty_block and n >= 96:
        src = np.where((src >= 32) & (src < 64), src + 32, src)   # rows 32..63 stay empty
    if self_loops:
        k = min(e, 16)
        dst[:k] = src[:k]
    if dup and e:
        idx = rng.integers(0, e, size=max(1, e // 10))
        src = np.concatenate([src, src[idx], src[idx[::2]], src[idx[::4]]])
        dst = np.concatenate([dst, dst[idx], dst[idx[::2]], dst[idx[::4]]])
    return src, dst


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("n", [1, 31, 32, 33, 127, 129, 1213, 4097])
@pytest.mark.parametrize("density", [0.0, 0.02, 2.0])
def test_format_matches_the_numpy_model(qgtc, n, density):
    import torch

    rng = np.random.default_rng(n * 7 + int(density * 100))
    e = int(density * n * 4)
    src, dst = random_edges(rng, n, e)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    row_ptr, kquad, tiles = np_tiled(src, dst, n)
    assert isinstance(adj, qgtc.TiledAdjacency) and adj.n == n
    assert adj.n_tiles == kquad.size
    np.testing.assert_array_equal(adj.row_ptr.cpu().numpy(), row_ptr)
    np.testing.assert_array_equal(adj.kquad.cpu().numpy(), kquad)
    np.testing.assert_array_equal(adj.tiles.cpu().numpy().view(np.uint32), tiles)
    assert adj.nbytes == 8 * row_ptr.size + 4 * kquad.size + 512 * kquad.size
    assert adj.max_block_tiles == (int(np.diff(row_ptr).max()) if row_ptr.size > 1 else 0)
    # the dense words of the same edge list
    dense = qgtc.pack_edges(_dev(torch, src), _dev(torch, dst), n, n, 1)
    assert torch.equal(adj.to_rows(), dense)


def test_multiplicities_quantise_like_pack_edges(qgtc):
    import torch

    n = 300
    src = np.array([5] * 1 + [6] * 2 + [7] * 3 + [8] * 4 + [299] * 2 + [299], dtype=np.int64)
    dst = np.array([9] * 1 + [9] * 2 + [9] * 3 + [9] * 4 + [299] * 2 + [0], dtype=np.int64)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    rows = to_np_u32(adj.to_rows()).reshape(P8(n), S128(n) * 4)
    bit = lambda r, c: (rows[r, c // 32] >> (31 - c % 32)) & 1   # noqa: E731
    assert [bit(r, 9) for r in (5, 6, 7, 8)] == [1, 0, 1, 1]
    assert bit(299, 299) == 0 and bit(299, 0) == 1
    assert adj.n_tiles == 2   # row block 0 / k-quad 0 and row block 9 / k-quad 0; (299, 299) is a 2-fold edge: no tile of its own
    np.testing.assert_array_equal(adj.row_ptr.cpu().numpy()[[0, 1, 9, 10]], [0, 1, 1, 2])


def test_no_edges_and_all_cancelled(qgtc):
    import torch

    for src, dst in ((np.zeros(0, np.int64), np.zeros(0, np.int64)), (np.array([3, 3], np.int64), np.array([4, 4], np.int64))):
        adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), 100)
        assert adj.n_tiles == 0 and adj.tiles.shape == (0, 32, 4)
        np.testing.assert_array_equal(adj.row_ptr.cpu().numpy(), np.zeros(5, np.int64))
        X = qgtc.val2bit(torch.ones(100, 20, device="cuda"), 2, True, False)
        assert not qgtc.tiledMM2Bit(adj, X, 20, 2, 3).any()
        assert not qgtc.tiledMM2Int(adj, X, 20, 2).any()


def test_bad_indices_raise_or_are_skipped(qgtc):
    import torch

    n = 200
    src = np.array([0, 5, -1, 3, 199, 200, 7], dtype=np.int64)
    dst = np.array([1, 6, 2, -4, 199, 1, 1000], dtype=np.int64)
    with pytest.raises(RuntimeError, match="out of range"):
        qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n, validate=False)
    row_ptr, kquad, tiles = np_tiled(src, dst, n)
    np.testing.assert_array_equal(adj.row_ptr.cpu().numpy(), row_ptr)
    np.testing.assert_array_equal(adj.kquad.cpu().numpy(), kquad)
    np.testing.assert_array_equal(adj.tiles.cpu().numpy().view(np.uint32), tiles)
    assert torch.equal(adj.to_rows(), qgtc.pack_edges(_dev(torch, src), _dev(torch, dst), n, n, 1, False))


# (n, N, w, ob): every N of {1, 10, 16, 24, 33, 64, 128, 256, 602, 1024} (every kernel variant), every w of {1, 2, 3, 4, 5, 8}, every ob
# of {1, 2, 3, 4, 8, 16, 32}
PRODUCTS = [
    (1, 1, 1, 1),
    (33, 10, 2, 2),
    (129, 16, 3, 4),
    (1213, 33, 4, 8),
    (4097, 64, 8, 16),
    (20000, 128, 2, 32),
    (5000, 256, 1, 1),
    (3000, 602, 4, 2),
    (2000, 1024, 8, 8),
    (20000, 16, 4, 4),
    (777, 1024, 1, 32),
    (9000, 602, 3, 16),
    (300, 24, 5, 3),
]


def _features(torch, rng, n, N, w):
    return torch.from_numpy(rng.integers(0, 2 ** w, size=(n, N)).astype(np.float32)).cuda()


@pytest.mark.parametrize("n,N,w,ob", PRODUCTS)
def test_products_equal_the_dense_route(qgtc, n, N, w, ob):
    import torch

    rng = np.random.default_rng(n + N + w + ob)
    src, dst = random_edges(rng, n, 6 * n + 5)
    dsrc, ddst = _dev(torch, src), _dev(torch, dst)
    adj = qgtc.pack_edges_tiled(dsrc, ddst, n)
    A = qgtc.pack_edges(dsrc, ddst, n, n, 1)
    X = qgtc.val2bit(_features(torch, rng, n, N, w), w, True, False)
    got_b = qgtc.tiledMM2Bit(adj, X, N, w, ob)
    got_f = qgtc.tiledMM2Int(adj, X, N, w)
    assert got_b.shape == (ob * P8(n), S128(N) * 4) and got_f.shape == (n, N) and got_f.dtype == torch.float32
    for eng in ENGINES:
        with use_engine(qgtc, eng):
            assert torch.equal(got_b, qgtc.bitMM2Bit(A, X, n, n, N, 1, w, ob)), eng
            assert torch.equal(got_f, qgtc.bitMM2Int(A, X, n, n, N, 1, w, True)), eng
            # the tiled entry takes no notice of the engine
            assert torch.equal(qgtc.tiledMM2Bit(adj, X, N, w, ob), got_b)


@pytest.mark.parametrize("n,N,w,ob", [(40, 10, 2, 3), (300, 64, 4, 8), (161, 130, 8, 32)])
def test_products_equal_the_oracle(qgtc, oracle, n, N, w, ob):
    import torch

    rng = np.random.default_rng(n)
    src, dst = random_edges(rng, n, 5 * n)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    Asum = np.zeros((n, n), dtype=np.float32)
    np.add.at(Asum, (src, dst), 1.0)
    Xf = rng.integers(0, 2 ** w, size=(n, N)).astype(np.float32)
    oA, oX = oracle.val2bit(Asum, 1), oracle.val2bit(Xf, w, True)
    X = qgtc.val2bit(torch.from_numpy(Xf).cuda(), w, True, False)
    np.testing.assert_array_equal(to_np_u32(qgtc.tiledMM2Bit(adj, X, N, w, ob)), oracle.bitmm2bit(oA, oX, n, n, N, 1, w, ob))
    np.testing.assert_array_equal(qgtc.tiledMM2Int(adj, X, N, w).cpu().numpy(), oracle.bitmm2int(oA, oX, n, n, N, 1, w, True))


def test_hub_row_sums_past_two_to_the_24(qgtc):
    import torch

    n, N, hub = 70000, 40, 12345
    rng = np.random.default_rng(5)
    src = np.concatenate([np.full(n, hub, np.int64), rng.integers(0, n, size=3 * n, dtype=np.int64)])
    dst = np.concatenate([np.arange(n, dtype=np.int64), rng.integers(0, n, size=3 * n, dtype=np.int64)])
    keep = src != hub
    keep[:n] = True                                   # the hub row: every node exactly once
    src, dst = src[keep], dst[keep]
    dsrc, ddst = _dev(torch, src), _dev(torch, dst)
    adj = qgtc.pack_edges_tiled(dsrc, ddst, n)
    X = qgtc.val2bit(torch.full((n, N), 255.0, device="cuda"), 8, True, False)
    f = qgtc.tiledMM2Int(adj, X, N, 8)
    assert (f[hub] == 17850000.0).all()
    b = qgtc.tiledMM2Bit(adj, X, N, 8, 32)
    words = to_np_u32(b).reshape(32, P8(n), S128(N) * 4)
    col0 = [(int(words[p, hub, 0]) >> 31) & 1 for p in range(32)]
    assert sum(v << p for p, v in enumerate(col0)) == 17850000
    A = qgtc.pack_edges(dsrc, ddst, n, n, 1)
    assert torch.equal(f, qgtc.bitMM2Int(A, X, n, n, N, 1, 8, True))
    assert torch.equal(b, qgtc.bitMM2Bit(A, X, n, n, N, 1, 8, 32))


def _reddit_sized():
    from qgtc_ppopp22_amd.graph import make_sbm_graph

    return make_sbm_graph("reddit-sized", 232965, 1500, 20.0, 8, seed=4)


def test_beyond_the_dense_cap(qgtc):
    """232 965 nodes: the dense operand would be 6.8 GB (over the 4 GiB cap); 32 aligned 1024-row slices of the tiled product
    equal the dense product of the slice's own rows."""
    import torch

    g = _reddit_sized()
    n, N, w, ob = g.n_nodes, 64, 2, 4
    dsrc, ddst = _dev(torch, g.src), _dev(torch, g.dst)
    adj = qgtc.pack_edges_tiled(dsrc, ddst, n)
    rng = np.random.default_rng(8)
    X = qgtc.val2bit(_features(torch, rng, n, N, w), w, True, False)
    out_b = qgtc.tiledMM2Bit(adj, X, N, w, ob).view(ob, P8(n), S128(N) * 4)
    out_f = qgtc.tiledMM2Int(adj, X, N, w)
    starts = rng.choice(n // 1024, size=32, replace=False) * 1024
    for r0 in starts.tolist():
        sel = (dsrc >= r0) & (dsrc < r0 + 1024)
        A = qgtc.pack_edges((dsrc[sel] - r0).contiguous(), ddst[sel].contiguous(), 1024, n, 1)
        want_b = qgtc.bitMM2Bit(A, X, 1024, n, N, 1, w, ob).view(ob, 1024, S128(N) * 4)
        assert torch.equal(out_b[:, r0:r0 + 1024], want_b), r0
        assert torch.equal(out_f[r0:r0 + 1024], qgtc.bitMM2Int(A, X, 1024, n, N, 1, w, True)), r0


@pytest.mark.parametrize("n", [300, 4096])
def test_module_tiled_equals_edge_list(qgtc, n):
    import torch

    from qgtc_ppopp22_amd.conv import GCNConv_Qnt

    torch.manual_seed(0)
    rng = np.random.default_rng(n)
    src, dst = random_edges(rng, n, 8 * n)
    dsrc, ddst = _dev(torch, src), _dev(torch, dst)
    m = GCNConv_Qnt(48, 64, 10, w_bit=2, act_bit=3).cuda()
    X = torch.randn(n, 48, device="cuda")
    want = m((dsrc, ddst, n), X)
    got = m(qgtc.pack_edges_tiled(dsrc, ddst, n), X)
    assert got.dtype == torch.float32 and got.shape == (n, 10)
    assert torch.equal(got, want)


def test_module_runs_on_a_reddit_sized_graph(qgtc):
    import torch

    from qgtc_ppopp22_amd.conv import GCNConv_Qnt

    g = _reddit_sized()
    torch.manual_seed(1)
    m = GCNConv_Qnt(8, 32, 41, w_bit=2, act_bit=2).cuda()
    adj = qgtc.pack_edges_tiled(_dev(torch, g.src), _dev(torch, g.dst), g.n_nodes)
    out = m(adj, torch.from_numpy(g.feat).cuda())
    assert out.dtype == torch.float32 and out.shape == (g.n_nodes, 41)
    assert torch.isfinite(out).all()
