"""Node masks on the quantised tiled products on the device (``row_mask=`` / ``nbr_mask=`` of QGTC.tiledMM2Bit / QGTC.tiledMM2Int,
``nodes=`` of conv.GCNConv_Qnt and the four C entries of include/qgtc_bitnodes.h) against tests/tiled_bit_nodes_model.py: masking is
restricting the edge list, so every masked product must give, bit for bit, what the exact models give on the induced edges and what the
unmasked product gives on ``pack_edges_tiled`` of the induced edges. Nothing is sampled and no tolerance is used."""
import ctypes

import numpy as np
import pytest

import dirty_memory as dmem
import tiled_bit_nodes_model as bn
import tiled_nodes_model as nm
from helpers import to_np_u32
from qgtc_ppopp22_amd.tiled import node_bitmap
from tiled_model import random_edges
from tiled_scaled_model import mean_scale

pytestmark = pytest.mark.gpu

MODULE = "tests/test_tiled_bit_nodes_gpu.py"
NO_EDGES = (np.zeros(0, np.int64), np.zeros(0, np.int64))
CANARY = 64


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits_of(qgtc, torch, Xq, w):
    """X in the cols layout [w][PAD128(N)][S128(n) * 4], from the quantised features"""
    return qgtc.val2bit(torch.from_numpy(np.ascontiguousarray(Xq, dtype=np.float32)).cuda(), w, True, False)


def _bm(torch, flags, n):
    return None if flags is None else node_bitmap(_dev(torch, flags), n)


def _filled_edges(rng, n, e):
    """random_edges (hubs, loops, duplicates) plus uniform edges, so that no row block or k-quad is left empty"""
    src, dst = random_edges(rng, n, e)
    return (np.concatenate([src, rng.integers(0, n, size=e, dtype=np.int64)]),
            np.concatenate([dst, rng.integers(0, n, size=e, dtype=np.int64)]))


def _check(torch, qgtc, oracle, src, dst, n, N, R, S, Xq, bit2, ob, what, adj=None, repack=True, seed=0):
    """both views under (R, S), which are relative to the view; the plain sum, the induced mean and a random positive row scale;
    tiledMM2Bit and tiledMM2Int - against the models on the induced edges and, with `repack`, against the unmasked operators on the
    adjacency packed from the induced edges"""
    adj = adj if adj is not None else qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    X = _bits_of(qgtc, torch, Xq, bit2)
    kw = {"row_mask": _bm(torch, R, n), "nbr_mask": _bm(torch, S, n)}
    random_scale = np.random.default_rng(seed + n).uniform(2.0 ** -10, 4.0, n).astype(np.float32)
    for transposed in (False, True):
        a = adj.T if transposed else adj
        w = f"{what} {'adj.T' if transposed else 'adj'}"
        C = bn.sums(src, dst, n, Xq, R, S, transposed)
        deg = bn.sums(src, dst, n, np.ones((n, 1), np.int64), R, S, transposed)[:, 0]
        induced_mean = a.mean_scale(**kw)
        np.testing.assert_array_equal(induced_mean.cpu().numpy().view(np.uint32), mean_scale(deg).view(np.uint32), err_msg=w)
        ka = None
        if repack:
            ks, kd = nm.induced_edges(src, dst, n, R, S, transposed)
            kadj = qgtc.pack_edges_tiled(_dev(torch, ks), _dev(torch, kd), n)
            ka = kadj.T if transposed else kadj
        for name, scale, dscale in (("sum", None, None), ("mean", mean_scale(deg), induced_mean), ("scaled", random_scale, _dev(torch, random_scale))):
            floats, bits = bn.reference(oracle, C, ob, scale)
            got_b = qgtc.tiledMM2Bit(a, X, N, bit2, ob, dscale, **kw)
            got_f = qgtc.tiledMM2Int(a, X, N, bit2, dscale, **kw)
            assert got_b.dtype == torch.int32 and tuple(got_b.shape) == (ob * ((n + 7) // 8 * 8), (N + 127) // 128 * 4)
            assert got_f.dtype == torch.float32 and tuple(got_f.shape) == (n, N)
            np.testing.assert_array_equal(to_np_u32(got_b), bits, err_msg=f"{w} {name}: bits against the model")
            np.testing.assert_array_equal(to_np_u32(got_f), floats.view(np.uint32).reshape(-1), err_msg=f"{w} {name}: floats against the model")
            if ka is not None:
                assert torch.equal(got_b, qgtc.tiledMM2Bit(ka, X, N, bit2, ob, dscale)), f"{w} {name}: bits against the re-packed adjacency"
                assert torch.equal(got_f.view(torch.int32), qgtc.tiledMM2Int(ka, X, N, bit2, dscale).view(torch.int32)), \
                    f"{w} {name}: floats against the re-packed adjacency"
            if R is not None and name != "scaled":                # rows outside the row mask: 0 in every plane, +0 as a float
                assert (to_np_u32(got_f).reshape(n, N)[~R] == 0).all(), w
    return adj


# ---- 1. the sweep ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,N,kind", bn.SWEEP, ids=[f"n{n}-N{N}-{k}" for n, N, k in bn.SWEEP])
def test_masked_products_equal_the_model_and_the_repacked_adjacency(qgtc, oracle, n, N, kind):
    import torch

    adj = None
    for bit2, ob in bn.bit_pairs(n, N):
        src, dst, R, S, Xq = bn.inputs(n, N, kind, bit2)
        adj = _check(torch, qgtc, oracle, src, dst, n, N, R, S, Xq, bit2, ob, f"n={n} N={N} {kind} bits=({bit2}, {ob})", adj=adj)


# ---- 2. the edges of the mask -----------------------------------------------------------------------------------------------------------------
def _between(n, lo, hi):
    f = np.zeros(n, bool)
    f[lo:hi] = True
    return f


EDGE_MASKS = {
    "empty": lambda n: np.zeros(n, bool),
    "one node": lambda n: _between(n, 70, 71),
    "ends on a 32-boundary": lambda n: _between(n, 5, 64),
    "starts on a 32-boundary": lambda n: _between(n, 64, 91),
    "ends on a 128-boundary": lambda n: _between(n, 100, 256),
    "starts on a 128-boundary": lambda n: _between(n, 128, 140),
    "the last, partial block alone": lambda n: _between(n, n - 1, n),
}


@pytest.mark.parametrize("which", sorted(EDGE_MASKS))
def test_edge_masks(qgtc, oracle, which):
    """Each special set as the row mask alone, as the neighbour mask alone (under a random other mask), and as both; n = 333 has a last
    block of 13 rows and a last k-quad of 77."""
    import torch

    n, N = 333, 40
    bit2, ob = bn.BITS
    rng = np.random.default_rng(len(which))
    src, dst = _filled_edges(rng, n, 4 * n)
    Xq = rng.integers(0, 2 ** bit2, size=(n, N))
    f = EDGE_MASKS[which](n)
    other = rng.random(n) < 0.5
    adj = None
    for R, S in ((f, None), (None, f), (f, other), (other, f), (f, f)):
        adj = _check(torch, qgtc, oracle, src, dst, n, N, R, S, Xq, bit2, ob, which, adj=adj)


@pytest.mark.parametrize("n,N", [(1, 5), (300, 24), (300, 130)])
def test_a_graph_without_edges(qgtc, oracle, n, N):
    import torch

    bit2, ob = bn.BITS
    rng = np.random.default_rng(n + N)
    Xq = rng.integers(0, 2 ** bit2, size=(n, N))
    for R, S in ((np.ones(n, bool), np.ones(n, bool)), (rng.random(n) < 0.5, None), (None, np.zeros(n, bool))):
        _check(torch, qgtc, oracle, *NO_EDGES, n, N, R, S, Xq, bit2, ob, f"no edges n={n}")


@pytest.mark.parametrize("N", [24, 130])
def test_all_ones_masks_and_one_null_give_the_plain_words(qgtc, N):
    import torch

    n = 333
    bit2, ob = bn.BITS
    rng = np.random.default_rng(2)
    src, dst = random_edges(rng, n, 6 * n + 5)
    X = _bits_of(qgtc, torch, rng.integers(0, 2 ** bit2, size=(n, N)), bit2)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    ones = _bm(torch, np.ones(n, bool), n)
    scale = _dev(torch, rng.uniform(0.25, 2.0, n).astype(np.float32))
    for a in (adj, adj.T):
        for sc in (None, scale):
            plain_b, plain_f = qgtc.tiledMM2Bit(a, X, N, bit2, ob, sc), qgtc.tiledMM2Int(a, X, N, bit2, sc)
            for rm, sm in ((ones, ones), (ones, None), (None, ones)):
                assert torch.equal(qgtc.tiledMM2Bit(a, X, N, bit2, ob, sc, row_mask=rm, nbr_mask=sm), plain_b)
                assert torch.equal(qgtc.tiledMM2Int(a, X, N, bit2, sc, row_mask=rm, nbr_mask=sm).view(torch.int32), plain_f.view(torch.int32))


# ---- 3. skipped blocks read nothing -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [8, 40, 130])
def test_dead_blocks_and_dead_neighbours_are_never_read(qgtc, N):
    """Wrong VALUES where the contract says nothing is read, never a wrong index: the tiles of dead row blocks (32 rows on adj; on adj.T
    the 128 rows of a dead k-quad) are overwritten with all-ones words and X's words of dead neighbours (a dead k-quad's four words of
    every line on adj, a dead row block's word on adj.T) with random words. Every row_ptr, kquad and column index entry stays as it is.
    The masked outputs do not change."""
    import torch

    n = 1000
    bit2, ob = bn.BITS
    rng = np.random.default_rng(N)
    src, dst = _filled_edges(rng, n, 4 * n)
    quad = np.arange(n) // 128
    R = np.isin(quad, (1, 4, 6)) & (rng.random(n) < 0.5)       # whole k-quads (so whole row blocks) without a live row
    S = np.isin(quad, (0, 2, 5)) & (rng.random(n) < 0.5)       # whole k-quads (so whole row blocks) without a live neighbour
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    X = _bits_of(qgtc, torch, rng.integers(0, 2 ** bit2, size=(n, N)), bit2)
    words = adj.mask_words
    Xv = X.view(bit2, -1, words)
    kw = {"row_mask": _bm(torch, R, n), "nbr_mask": _bm(torch, S, n)}
    row_ptr, kquad = adj.row_ptr.cpu().numpy(), adj.kquad.cpu().numpy()
    tile_rb = np.repeat(np.arange(row_ptr.size - 1), np.diff(row_ptr))
    for transposed in (False, True):
        a = adj.T if transposed else adj
        want_b, want_f = qgtc.tiledMM2Bit(a, X, N, bit2, ob, **kw), qgtc.tiledMM2Int(a, X, N, bit2, **kw)
        if transposed:
            dead_tiles = ~np.isin(kquad, (1, 4, 6))                              # the tiles of the k-quads without a live output row
            dead_words = np.flatnonzero(~np.isin(np.arange(words) // 4, (0, 2, 5)))   # X's word rb of a row block without a live neighbour
        else:
            dead_tiles = ~np.isin(tile_rb // 4, (1, 4, 6))                        # the tiles of the row blocks without a live row
            dead_words = np.flatnonzero(~np.isin(np.arange(words) // 4, (0, 2, 5)))   # X's four words of a k-quad without a live neighbour
        assert dead_tiles.any() and not dead_tiles.all() and dead_words.size
        tiles = adj.tiles.clone()
        tiles.view(-1, 128)[_dev(torch, np.flatnonzero(dead_tiles))] = -1
        X2 = X.clone()
        junk = _dev(torch, rng.integers(-2 ** 31, 2 ** 31, size=(bit2, Xv.shape[1], dead_words.size)).astype(np.int32))
        X2.view(bit2, -1, words)[:, :, _dev(torch, dead_words)] = junk
        bad = qgtc.TiledAdjacency(n, adj.row_ptr, adj.kquad, tiles)
        b = bad.T if transposed else bad
        assert not torch.equal(qgtc.tiledMM2Int(b, X2, N, bit2), qgtc.tiledMM2Int(a, X, N, bit2)), "the overwritten values matter unmasked"
        assert torch.equal(qgtc.tiledMM2Bit(b, X2, N, bit2, ob, **kw), want_b), f"bits transposed={transposed}"
        assert torch.equal(qgtc.tiledMM2Int(b, X2, N, bit2, **kw).view(torch.int32), want_f.view(torch.int32)), f"floats transposed={transposed}"


# ---- 4. every output word is written --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,N", [(333, 24), (1000, 130)])
def test_on_recycled_poisoned_memory(qgtc, oracle, n, N):
    """The masked outputs come from torch.empty: on memory whose every word is a poison pattern (tests/dirty_memory.py) the rows of dead
    blocks, the pad rows up to PAD8(n) and the columns past N hold what the model says (zeros), under both patterns."""
    import torch

    bit2, ob = bn.BITS
    rng = np.random.default_rng(n + N)
    src, dst = _filled_edges(rng, n, 4 * n)
    Xq = rng.integers(0, 2 ** bit2, size=(n, N))
    R = (np.arange(n) // 128 % 2 == 1) & (rng.random(n) < 0.5)     # every other k-quad, so three of four row blocks, is dead
    S = rng.random(n) < 0.5
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    adj.T
    X = _bits_of(qgtc, torch, Xq, bit2)
    rm, sm = _bm(torch, R, n), _bm(torch, S, n)
    scale = _dev(torch, rng.uniform(0.25, 2.0, n).astype(np.float32))
    dev = torch.device("cuda", torch.cuda.current_device())

    def run():
        out = []
        for a in (adj, adj.T):
            for sc in (None, scale):
                out += [qgtc.tiledMM2Bit(a, X, N, bit2, ob, sc, row_mask=rm, nbr_mask=sm), qgtc.tiledMM2Int(a, X, N, bit2, sc, row_mask=rm, nbr_mask=sm)]
        return out

    want = []
    for transposed in (False, True):
        C = bn.sums(src, dst, n, Xq, R, S, transposed)
        for sc in (None, scale.cpu().numpy()):
            floats, bits = bn.reference(oracle, C, ob, sc)
            want += [bits.view(np.int32).reshape(ob * ((n + 7) // 8 * 8), -1), floats]
    run()                                          # warm-up outside the poisoned region: code objects are loaded
    results = []
    for pattern in dmem.PATTERNS:
        with dmem.dirty(torch, dev, pattern, inputs=[X, rm, sm, scale]) as d:
            dmem.announce(MODULE, d)
            got = [t.cpu() for t in run()]
        dmem.same_as_model(got, want, f"masked bit products on memory poisoned with {pattern:#010x}")
        results.append(got)
    dmem.same_bits(results[0], results[1], "one pattern against the other")


@pytest.mark.parametrize("n,N", [(97, 17), (333, 130)])
def test_the_c_entries_stay_within_their_outputs_and_ignore_pad_bits(qgtc, oracle, n, N):
    """The four entries through ctypes, into poisoned outputs with canaries behind them, from HAND-MADE bitmaps whose pad bits (the
    positions from n up) are all set; one mask alone and none (a NULL is all nodes); with and without a row_scale."""
    import torch

    from qgtc_ppopp22_amd import cabi

    L = cabi.load()
    bit2, ob = bn.BITS
    rng = np.random.default_rng(n)
    src, dst = random_edges(rng, n, 6 * n + 5)
    Xq = rng.integers(0, 2 ** bit2, size=(n, N))
    Rf, Sf = rng.random(n) < 0.5, rng.random(n) < 0.5
    words = nm.bitmap_words(n)

    def dirty(flags):
        padded = np.ones(words * 32, bool)
        padded[:n] = flags
        w = nm.bitmap(padded)
        assert (nm.members(w, n) == flags).all() and (w != nm.bitmap(flags)).any()
        return _dev(torch, w.view(np.int32))

    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    X = _bits_of(qgtc, torch, Xq, bit2)
    scale_np = rng.uniform(0.25, 2.0, n).astype(np.float32)
    scale = _dev(torch, scale_np)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rm, sm = dirty(Rf), dirty(Sf)
    n_words, n_elems = ob * ((n + 7) // 8 * 8) * ((N + 127) // 128 * 4), n * N
    for transposed in (False, True):
        t = adj.T
        idx = (t.col_ptr.data_ptr(), t.col_tile.data_ptr(), t.col_rb.data_ptr(), adj.tiles.data_ptr()) if transposed else \
            (adj.row_ptr.data_ptr(), adj.kquad.data_ptr(), adj.tiles.data_ptr())
        sfx = "_t_nodes" if transposed else "_nodes"
        head = (*idx, adj.n_tiles, n, X.data_ptr(), X.numel(), N, bit2)
        for R, S, masks in ((Rf, Sf, (rm.data_ptr(), sm.data_ptr(), words)), (Rf, None, (rm.data_ptr(), None, words)),
                            (None, Sf, (None, sm.data_ptr(), words)), (None, None, (None, None, 0))):
            C = bn.sums(src, dst, n, Xq, R, S, transposed)
            for sc, dsc in ((None, None), (scale_np, scale.data_ptr())):
                floats, bits = bn.reference(oracle, C, ob, sc)
                out = torch.full((n_words + CANARY,), -0x5A5A5A5B, dtype=torch.int32, device="cuda")
                assert getattr(L, "qgtc_tiledmm2bit" + sfx)(*head, ob, dsc, out.data_ptr(), n_words, *masks, st) == 0
                got = to_np_u32(out)
                np.testing.assert_array_equal(got[:n_words], bits, err_msg=f"C bits transposed={transposed}")
                assert (got[n_words:] == np.uint32(0xA5A5A5A5)).all(), "bit canaries"
                outf = torch.full((n_elems + CANARY,), float("nan"), dtype=torch.float32, device="cuda")
                assert getattr(L, "qgtc_tiledmm2int" + sfx)(*head, dsc, outf.data_ptr(), n_elems, *masks, st) == 0
                gotf = to_np_u32(outf)
                np.testing.assert_array_equal(gotf[:n_elems], floats.view(np.uint32).reshape(-1), err_msg=f"C floats transposed={transposed}")
                assert (gotf[n_elems:] == 0x7FC00000).all(), "float canaries"
    torch.cuda.synchronize()


# ---- 5. the Python refusals ---------------------------------------------------------------------------------------------------------------------
def test_a_bad_mask_raises_what_tiledmmfloat_raises(qgtc):
    import torch

    n, N = 100, 8
    bit2, ob = bn.BITS
    rng = np.random.default_rng(0)
    src, dst = random_edges(rng, n, 300)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    Xq = rng.integers(0, 2 ** bit2, size=(n, N))
    X, Xf = _bits_of(qgtc, torch, Xq, bit2), _dev(torch, Xq.astype(np.float32))
    mask = torch.zeros(4, dtype=torch.int32, device="cuda")
    bad_masks = (mask.tolist(), mask.to(torch.int64), mask[:-1], torch.zeros(8, dtype=torch.int32, device="cuda"),
                 torch.zeros(8, dtype=torch.int32, device="cuda")[::2], mask.cpu(), mask.to("meta"))
    for a in (adj, adj.T):
        for name in ("row_mask", "nbr_mask"):
            for bad in bad_masks:
                with pytest.raises((TypeError, ValueError)) as want:
                    qgtc.tiledMMFloat(a, Xf, **{name: bad})
                for call in (lambda **kw: qgtc.tiledMM2Bit(a, X, N, bit2, ob, **kw), lambda **kw: qgtc.tiledMM2Int(a, X, N, bit2, **kw)):
                    with pytest.raises(type(want.value)) as got:
                        call(**{name: bad})
                    assert str(got.value) == str(want.value)
    # a row_scale is checked as in the unmasked call
    with pytest.raises(TypeError, match="row_scale must be float32"):
        qgtc.tiledMM2Int(adj, X, N, bit2, torch.zeros(n, dtype=torch.float64, device="cuda"), row_mask=mask)
    with pytest.raises(TypeError, match="TiledAdjacency"):
        qgtc.tiledMM2Int(None, X, N, bit2, row_mask=mask)


# ---- 6. the layer -------------------------------------------------------------------------------------------------------------------------------
def _same(torch, a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("aggr,float_out", [("sum", False), ("sum", True), ("mean", False), ("mean", True)])
def test_gcnconv_qnt_on_the_induced_subgraph(qgtc, aggr, float_out):
    """``nodes=`` as a bool vector on adj, adj.T and a reordered adjacency: every row equals the same layer on the re-packed induced
    adjacency (rows outside ``nodes`` are isolated nodes there), and the masks change the result."""
    import torch

    from qgtc_ppopp22_amd import conv

    n, F_in, H, C = 333, 12, 20, 7
    rng = np.random.default_rng(21)
    src, dst = random_edges(rng, n, 6 * n + 5)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    X = _dev(torch, rng.uniform(0.0, 8.0, (n, F_in)).astype(np.float32))
    nodes = rng.random(n) < 0.5
    dn = _dev(torch, nodes)
    torch.manual_seed(0)
    layer = conv.GCNConv_Qnt(F_in, H, C, aggr=aggr, float_out=float_out).cuda()
    ks, kd = nm.induced_edges(src, dst, n, nodes, nodes, False)
    kadj = qgtc.pack_edges_tiled(_dev(torch, ks), _dev(torch, kd), n)
    for a, ka in ((adj, kadj), (adj.T, kadj.T)):
        got, want = layer(a, X, nodes=dn), layer(ka, X)
        assert got.dtype == torch.float32 and tuple(got.shape) == (n, C)
        assert _same(torch, got[dn], want[dn]), "the rows of nodes"
        assert _same(torch, got, want), "rows outside nodes are what the layer gives an isolated node"
        assert not _same(torch, got, layer(a, X)), "the masks change the result"
    # a reordered adjacency: `nodes` stays in X's numbering and the layer moves it; the re-packed induced adjacency in the same numbering
    re = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n, reorder=True)
    rank = re.rank.cpu().numpy()
    assert (rank != np.arange(n)).any()
    raw = qgtc.pack_edges_tiled(_dev(torch, rank[ks]), _dev(torch, rank[kd]), n)
    kre = qgtc.TiledAdjacency(n, raw.row_ptr, raw.kquad, raw.tiles, re.perm, re.rank)
    for a, ka in ((re, kre), (re.T, kre.T)):
        got = layer(a, X, nodes=dn)
        assert _same(torch, got, layer(ka, X))
    if aggr == "sum" and not float_out:
        assert _same(torch, layer(re, X, nodes=dn), layer(adj, X, nodes=dn)), "reordering moves nothing"


def test_gcnconv_qnt_refuses_nodes_on_a_dense_adjacency(qgtc):
    import torch

    from qgtc_ppopp22_amd import conv

    n = 40
    layer = conv.GCNConv_Qnt(4, 4, 4).cuda()
    X = torch.ones((n, 4), device="cuda")
    nodes = torch.ones(n, dtype=torch.bool, device="cuda")
    with pytest.raises(NotImplementedError, match="nodes needs a QGTC.TiledAdjacency"):
        layer(torch.ones((n, n), device="cuda"), X, nodes=nodes)
    with pytest.raises(NotImplementedError, match="nodes needs a QGTC.TiledAdjacency"):
        layer((torch.zeros(3, dtype=torch.int64, device="cuda"), torch.zeros(3, dtype=torch.int64, device="cuda"), n), X, nodes=nodes)
    adj = qgtc.pack_edges_tiled(torch.zeros(3, dtype=torch.int64, device="cuda"), torch.arange(3, device="cuda"), n)
    with pytest.raises(TypeError, match="bool tensor"):
        layer(adj, X, nodes=torch.ones(n, device="cuda"))
