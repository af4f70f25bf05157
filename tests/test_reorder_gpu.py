"""Node reordering on the device (QGTC.reorder_nodes, pack_edges_tiled(reorder=True), TiledAdjacency.to_new / to_old /
to_old_packed, GCNConv_Qnt on a reordered adjacency): the permutation equals the NumPy model (tests/reorder_model.py) element for
element, it makes shuffled graphs compact again, and the products and the module give the unreordered results after the gathers."""

import numpy as np
import pytest

from reorder_model import reorder_model, shuffled_sbm, tile_count

pytestmark = pytest.mark.gpu


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).cuda()


def _star(rng):
    """A hub joined to 12 000 leaves (its list takes the workgroup path), leaves joined in small random groups."""
    n = 12001
    leaves = np.arange(1, n, dtype=np.int64)
    src = np.concatenate([np.zeros(n - 1, dtype=np.int64), rng.integers(1, n, 20000)])
    dst = np.concatenate([leaves, np.minimum(src[n - 1:] + rng.integers(1, 40, 20000), n - 1)])
    return src, dst, n


def _graph(name):
    rng = np.random.default_rng(11)
    if name.startswith("sbm"):
        n = int(name[3:])
        _, _, s, d = shuffled_sbm(n)
        return s, d, n
    if name == "deg20_sbm":            # lists of 17 .. 256 entries: the one-wave path
        _, _, s, d = shuffled_sbm(5000, deg=20.0)
        return s, d, 5000
    if name == "uniform":
        n = 5000
        return rng.integers(0, n, 35000), rng.integers(0, n, 35000), n
    if name == "dup_self":             # duplicates (each counts once), self loops (add nothing)
        n = 700
        s, d = rng.integers(0, n, 3000), rng.integers(0, n, 3000)
        s = np.concatenate([s, s[:500], s[:100], np.arange(0, n, 3)])
        d = np.concatenate([d, d[:500], d[:100], np.arange(0, n, 3)])
        return s, d, n
    if name == "isolated":             # an SBM on every third id of a larger range: two thirds of the nodes have no entries
        _, _, s, d = shuffled_sbm(1213)
        return 3 * s, 3 * d + 1, 3 * 1213 + 7
    if name == "empty":
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), 100
    if name == "star":
        return _star(rng)
    raise KeyError(name)


GRAPHS = ["sbm1", "sbm31", "sbm33", "sbm1213", "sbm20000", "deg20_sbm", "uniform", "dup_self", "isolated", "empty", "star"]


@pytest.mark.parametrize("sweeps,cap", [(20, 128), (0, 128), (1, 128), (2, 128), (20, 1)])
@pytest.mark.parametrize("name", GRAPHS)
def test_perm_equals_the_model(qgtc, name, sweeps, cap):
    import torch

    src, dst, n = _graph(name)
    want_perm, want_rank = reorder_model(src, dst, n, sweeps=sweeps, cap=cap)
    from qgtc_ppopp22_amd import load_ext

    perm, rank = load_ext()._reorder_nodes(_dev(torch, src), _dev(torch, dst), n, sweeps, cap, True)   # QGTC.reorder_nodes + rank
    assert perm.dtype == torch.int64 and perm.shape == (n,) and perm.device.type == "cuda"
    np.testing.assert_array_equal(perm.cpu().numpy(), want_perm)
    np.testing.assert_array_equal(rank.cpu().numpy(), want_rank)
    if sweeps == 20 and cap == 128:
        np.testing.assert_array_equal(qgtc.reorder_nodes(_dev(torch, src), _dev(torch, dst), n).cpu().numpy(), want_perm)


def test_two_calls_are_identical(qgtc):
    import torch

    src, dst, n = _graph("star")
    ds, dd = _dev(torch, src), _dev(torch, dst)
    a = qgtc.reorder_nodes(ds, dd, n, sweeps=12, cap=64)
    b = qgtc.reorder_nodes(ds, dd, n, sweeps=12, cap=64)
    assert torch.equal(a, b)


@pytest.mark.parametrize("n", [20000, 169343])
def test_quality_on_shuffled_sbm(qgtc, n):
    import torch

    s, d, ss, dd = shuffled_sbm(n)
    t_local = qgtc.pack_edges_tiled(_dev(torch, s), _dev(torch, d), n).n_tiles
    ds, dd_ = _dev(torch, ss), _dev(torch, dd)
    t_shuffled = qgtc.pack_edges_tiled(ds, dd_, n).n_tiles
    adj = qgtc.pack_edges_tiled(ds, dd_, n, reorder=True)
    assert adj.n_tiles <= 1.1 * t_local
    assert adj.n_tiles <= 0.25 * t_shuffled
    assert adj.n_tiles == tile_count(adj.rank.cpu().numpy()[ss], adj.rank.cpu().numpy()[dd], n)


def test_quality_on_a_uniform_graph(qgtc):
    import torch

    src, dst, n = _graph("uniform")
    ds, dd = _dev(torch, src), _dev(torch, dst)
    assert qgtc.pack_edges_tiled(ds, dd, n, reorder=True).n_tiles <= qgtc.pack_edges_tiled(ds, dd, n).n_tiles


def test_default_pack_is_unchanged(qgtc):
    import torch

    src, dst, n = _graph("sbm1213")
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    assert adj.perm is None and adj.rank is None
    X = torch.randn(n, 5, device="cuda")
    assert adj.to_new(X) is X and adj.to_old(X) is X
    assert adj.to_old_packed(X, 1) is X


def _vals(torch, rng, n, N, w):
    return torch.from_numpy(rng.integers(0, 2 ** w, size=(n, N)).astype(np.float32)).cuda()


@pytest.mark.parametrize("N,w,ob", [(16, 1, 1), (64, 2, 2), (33, 3, 5), (130, 4, 32)])
def test_products_in_the_new_numbering(qgtc, N, w, ob):
    import torch

    src, dst, n = _graph("sbm1213")
    src = np.concatenate([src, src[:50], src[:20], src[:20]])   # multiplicities 2 and 4 too
    dst = np.concatenate([dst, dst[:50], dst[:20], dst[:20]])
    ds, dd = _dev(torch, src), _dev(torch, dst)
    adj = qgtc.pack_edges_tiled(ds, dd, n)
    adj_r = qgtc.pack_edges_tiled(ds, dd, n, reorder=True)
    rank = adj_r.rank
    assert torch.equal(adj_r.perm[rank], torch.arange(n, device="cuda"))
    A_r = qgtc.pack_edges(rank[ds], rank[dd], n, n, 1)
    rng = np.random.default_rng(N + w + ob)
    X_old = _vals(torch, rng, n, N, w)
    X_new = adj_r.to_new(X_old)
    bx_new, bx_old = qgtc.val2bit(X_new, w, True, False), qgtc.val2bit(X_old, w, True, False)
    got_b = qgtc.tiledMM2Bit(adj_r, bx_new, N, w, ob)
    got_f = qgtc.tiledMM2Int(adj_r, bx_new, N, w)
    assert torch.equal(got_b, qgtc.bitMM2Bit(A_r, bx_new, n, n, N, 1, w, ob))
    assert torch.equal(got_f, qgtc.bitMM2Int(A_r, bx_new, n, n, N, 1, w, True))
    assert torch.equal(adj_r.to_old_packed(got_b, ob), qgtc.tiledMM2Bit(adj, bx_old, N, w, ob))
    assert torch.equal(adj_r.to_old(got_f), qgtc.tiledMM2Int(adj, bx_old, N, w))


@pytest.mark.parametrize("name", ["sbm1213", "star"])
def test_module_is_bit_identical_with_reorder(qgtc, name):
    import torch

    from qgtc_ppopp22_amd.conv import GCNConv_Qnt

    src, dst, n = _graph(name)
    ds, dd = _dev(torch, src), _dev(torch, dst)
    torch.manual_seed(0)
    m = GCNConv_Qnt(48, 64, 10, w_bit=2, act_bit=3).cuda()
    X = torch.randn(n, 48, device="cuda")
    want = m(qgtc.pack_edges_tiled(ds, dd, n), X)
    got = m(qgtc.pack_edges_tiled(ds, dd, n, reorder=True), X)
    assert got.shape == (n, 10)
    assert torch.equal(got, want)


def test_bad_indices_raise_or_are_skipped(qgtc):
    import torch

    src, dst, n = _graph("sbm1213")
    bad_s = np.concatenate([src, [n, -1, 5]])
    bad_d = np.concatenate([dst, [3, 4, n + 100]])
    ds, dd = _dev(torch, bad_s), _dev(torch, bad_d)
    with pytest.raises(RuntimeError, match="out of range"):
        qgtc.reorder_nodes(ds, dd, n)
    with pytest.raises(RuntimeError, match="out of range"):
        qgtc.reorder_nodes(ds, dd, n, sweeps=0)
    with pytest.raises(RuntimeError, match="out of range"):
        qgtc.pack_edges_tiled(ds, dd, n, reorder=True)
    want_perm, _ = reorder_model(bad_s, bad_d, n)
    np.testing.assert_array_equal(qgtc.reorder_nodes(ds, dd, n, validate=False).cpu().numpy(), want_perm)
    adj = qgtc.pack_edges_tiled(ds, dd, n, validate=False, reorder=True)
    good = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n, reorder=True)
    assert torch.equal(adj.perm, good.perm)
    assert torch.equal(adj.to_rows(), good.to_rows())


def test_c_abi_work_buffer(qgtc):
    """The entry through ctypes with raw device pointers: the size it asks for, a smaller buffer refused, and rank optional."""
    import torch

    from qgtc_ppopp22_amd import cabi

    L = cabi.load()
    src, dst, n = _graph("sbm1213")
    ds, dd = _dev(torch, src), _dev(torch, dst)
    e = src.size
    w0, w = L.qgtc_reorder_work_words(n, 0), L.qgtc_reorder_work_words(n, e)
    assert 0 < w0 < w and L.qgtc_reorder_work_words(2 * n, 0) > w0
    work = torch.empty(w, dtype=torch.int32, device="cuda")
    perm = torch.empty(n, dtype=torch.int64, device="cuda")
    bad = torch.ones(1, dtype=torch.int32, device="cuda")
    args = lambda words: (ds.data_ptr(), dd.data_ptr(), e, n, 20, 128, perm.data_ptr(), None, work.data_ptr(), words,  # noqa: E731
                          bad.data_ptr(), None)
    assert L.qgtc_reorder_nodes(*args(w - 1)) == 2   # QGTC_ESIZE
    assert L.qgtc_reorder_nodes(*args(w)) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(perm.cpu().numpy(), reorder_model(src, dst, n)[0])
    assert int(bad.item()) == 0
    # no edges: no work buffer needed, identity
    assert L.qgtc_reorder_nodes(None, None, 0, n, 20, 128, perm.data_ptr(), None, None, 0, None, None) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(perm.cpu().numpy(), np.arange(n))
