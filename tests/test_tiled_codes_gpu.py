"""The byte-code route of affine quantisation on the device (``affine.codes``, ``affine.tiledMMCodes``, ``affine.aggregate(route="bytes")``,
``affine.GCNConv_Affine(route="bytes")`` and the five C entries of include/qgtc_codes.h) against tests/tiled_codes_model.py and against the
planes route - ``val2bit_affine``, ``tiledMM2Int``, ``aggregate(route="planes")`` - on the same inputs. Every check is bit for bit
(tests/dirty_memory.py ``same_bits`` / ``same_as_model``); nothing is sampled and no tolerance is used. Both views throughout."""
import ctypes

import numpy as np
import pytest

import affine_model as am
import dirty_memory as dm
import tiled_codes_model as cm
import tiled_nodes_model as nm
from qgtc_ppopp22_amd.tiled import node_bitmap
from tiled_model import random_edges

pytestmark = pytest.mark.gpu
F32 = np.float32
CANARY = 64

# every named N with n = 300 (every width class, the chunk edge at 256, dwords that straddle N), every named n (block and k-quad edges)
# with N in {5, 64}: not the cross product
NS = (1, 3, 4, 5, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 300)
SIZES = (1, 31, 32, 33, 127, 128, 129, 300)
SHAPES = [(300, N) for N in NS] + [(n, N) for n in SIZES if n != 300 for N in (5, 64)]
LADDER = (1, 31, 32, 33, 64, 65, 97)      # neighbours of rows 0 .. 6: the queue's flush points and the remainders of the loads in flight


@pytest.fixture(scope="module")
def af(qgtc):
    from qgtc_ppopp22_amd import affine

    return affine


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cpu(ts):
    return [t.detach().cpu() for t in ts]


def _bm(flags, n):
    return None if flags is None else node_bitmap(_dev(flags), n)


def _random_graph(n, seed):
    """3 n random edges (hubs, loops, duplicates) and a self loop on every node"""
    src, dst = (np.asarray(a, dtype=np.int64) for a in random_edges(np.random.default_rng(seed), n, 3 * n))
    loops = np.arange(n, dtype=np.int64)
    return np.concatenate([src, loops]), np.concatenate([dst, loops])


def _ladder_graph(n, transposed, seed=7):
    """rows 0 .. 6 of the VIEW have exactly LADDER neighbours, spread over the whole graph; no other row has any"""
    rng = np.random.default_rng(seed)
    rows = np.concatenate([np.full(d, i, np.int64) for i, d in enumerate(LADDER)])
    cols = np.concatenate([np.sort(rng.choice(n, d, replace=False)).astype(np.int64) for d in LADDER])
    return (cols, rows) if transposed else (rows, cols)


def _hub_graph(n):
    """node 0 is adjacent to every node (itself included) and every node to node 0"""
    k = np.arange(n, dtype=np.int64)
    return np.concatenate([np.zeros(n, np.int64), k[1:]]), np.concatenate([k, np.zeros(n - 1, np.int64)])


def _features(n, N, seed):
    rng = np.random.default_rng(seed)
    T = (rng.normal(size=(n, N)) * 3.0 - 1.0).astype(F32)
    if n * N >= 8:
        T[rng.integers(0, n), rng.integers(0, N)] = np.nan
        T[rng.integers(0, n), rng.integers(0, N)] = np.inf
    return T


def _unpack_cols(words, bits, n, N):
    """the codes [n, N] held by cols-layout words [bits][PAD128(N)][S128(n) * 4]: element i of a line at word i >> 5, bit 31 - (i & 31)"""
    lines, lw = (N + 127) // 128 * 128, (n + 127) // 128 * 4
    w = np.ascontiguousarray(words).view(np.uint32).reshape(bits, lines, lw)
    b = np.unpackbits(w.astype(">u4").view(np.uint8).reshape(bits, lines, lw * 4), axis=2)
    assert not b[:, N:, :].any() and not b[:, :, n:].any()       # pad bits are zero
    return sum(b[p, :N, :n].astype(np.int64) << p for p in range(bits)).T


def _unpack_rows(words, bits, H, W):
    """the codes [H, W] held by rows-layout words [bits][PAD8(H)][S128(W) * 4]"""
    rows, rw = (H + 7) // 8 * 8, (W + 127) // 128 * 4
    w = np.ascontiguousarray(words).view(np.uint32).reshape(bits, rows, rw)
    b = np.unpackbits(w.astype(">u4").view(np.uint8).reshape(bits, rows, rw * 4), axis=2)
    return sum(b[p, :H, :W].astype(np.int64) << p for p in range(bits))


# ---- 1. the quantiser to bytes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_column", [False, True], ids=["tensor", "column"])
@pytest.mark.parametrize("shape", [(1, 1), (33, 7), (100, 64), (37, 130), (300, 5)], ids=str)
def test_codes_equal_the_model_and_the_unpacked_planes(af, shape, per_column):
    import torch

    H, W = shape
    x = _features(H, W, 11)
    dx = _dev(x)
    for bits in (1, 4, 8):
        qp = am.qparams(x, bits, per_column)
        dqp = af.qparams(dx, bits, per_column)
        dm.same_bits(_cpu([dqp]), [qp], f"qparams {shape} {bits}")
        q = af.codes(dx, bits, dqp)
        assert q.dtype == torch.uint8 and tuple(q.shape) == (H, W) and q.stride(1) == 1 and (H == 1 or q.stride(0) == cm.pad4(W))
        assert q.data_ptr() % 4 == 0
        whole = q.as_strided((H, cm.pad4(W)), (cm.pad4(W), 1))            # the buffer behind the view, pad bytes included
        dm.same_bits(_cpu([whole]), [cm.codes_buffer(x, qp, bits)], f"codes {shape} {bits} bits per_column={per_column}")
        words, _ = af.val2bit_affine(dx, bits, dqp, False, False)
        assert (_unpack_rows(words.cpu().numpy(), bits, H, W) == q.cpu().numpy()).all(), "the rows-layout planes hold other codes"
        words, _ = af.val2bit_affine(dx, bits, dqp, True, False)
        assert (_unpack_cols(words.cpu().numpy(), bits, H, W) == q.cpu().numpy()).all(), "the cols-layout planes hold other codes"


@pytest.mark.parametrize("W", [5, 64, 130])
def test_the_codes_entry_leaves_the_bytes_past_the_pad_alone(af, W):
    """qgtc_affine_codes called directly with ld = PAD4(W) + 8 into a buffer of canary bytes, x at an address that is 4- but not 16-byte
    aligned for the odd widths: codes, zeros up to PAD4(W), canaries beyond and around."""
    import torch
    from qgtc_ppopp22_amd import cabi

    H, bits, ld = 70, 8, cm.pad4(W) + 8
    x = _features(H, W, 12)
    holder = _dev(np.concatenate([np.zeros(1, F32), x.reshape(-1)]))
    dx = holder[1:].view(H, W)                                       # 4-byte aligned only
    lib = cabi.load()
    for per_column in (False, True):
        qp = am.qparams(x, bits, per_column)
        dqp = _dev(qp)
        buf = torch.full((CANARY + H * ld + CANARY,), 0xA5, dtype=torch.uint8, device="cuda")
        rc = lib.qgtc_affine_codes(dx.data_ptr(), H, W, bits, dqp.data_ptr(), qp.shape[0], buf.data_ptr() + CANARY, ld, (H - 1) * ld + cm.pad4(W),
                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
        got = buf.cpu().numpy()
        assert (got[:CANARY] == 0xA5).all() and (got[CANARY + H * ld:] == 0xA5).all()
        assert (got[CANARY:CANARY + H * ld].reshape(H, ld) == cm.codes_buffer(x, qp, bits, ld, 0xA5)).all()


# ---- 2. the sums and the fused aggregate --------------------------------------------------------------------------------------------------
def _check_view(af, qgtc, adj, src, dst, n, N, transposed, what, bits_list=(4, 8), seed=0, T=None):
    """one view: tiledMMCodes against the model and tiledMM2Int on the packed planes; aggregate(route="bytes") against the model and
    aggregate(route="planes"); unmasked, under two random halves, and with either mask alone; row_scale absent and present"""
    import torch

    a = adj.T if transposed else adj
    A = am.dense_view(src, dst, n, transposed)
    rng = np.random.default_rng(seed + 1000 * n + N)
    T = _features(n, N, seed + n + N) if T is None else T
    dT = _dev(T)
    R, S = rng.random(n) < 0.5, rng.random(n) < 0.5
    for rm, sm in ((None, None), (R, S), (R, None), (None, S)):
        kw = {"row_mask": _bm(rm, n), "nbr_mask": _bm(sm, n)}
        w = f"{what} masks=({rm is not None}, {sm is not None})"
        mean = am.inv_degree(am.masked_view(A, rm, sm).sum(axis=1))
        dmean = a.mean_scale(**kw)
        for bits in bits_list:
            qt = am.qparams(T, bits)
            Q = cm.codes(T, qt, bits)
            dqt = af.qparams(dT, bits)
            dQ = af.codes(dT, bits, dqt)
            got = af.tiledMMCodes(a, dQ, **kw)
            assert got.dtype == torch.int32 and tuple(got.shape) == (n, N)
            dm.same_as_model(_cpu([got]), [cm.tiled_mm_codes(A, Q, rm, sm)], f"tiledMMCodes {w} {bits} bits")
            planes, _ = af.val2bit_affine(dT, bits, dqt, True, False)
            assert torch.equal(got, qgtc.tiledMM2Int(a, planes, N, bits, None, **kw).to(torch.int32)), f"tiledMMCodes against tiledMM2Int {w}"
            for scale, dscale in ((None, None), (mean, dmean)):
                y = af.aggregate(a, dT, bits, dscale, route="bytes", **kw)
                assert y.dtype == torch.float32 and tuple(y.shape) == (n, N)
                dm.same_as_model(_cpu([y]), [cm.aggregate(A, T, bits, scale, rm, sm)], f"aggregate bytes {w} {bits} bits scaled={scale is not None}")
                dm.same_bits(_cpu([y]), _cpu([af.aggregate(a, dT, bits, dscale, route="planes", **kw)]),
                             f"aggregate bytes against planes {w} {bits} bits scaled={scale is not None}")


@pytest.mark.parametrize("n,N", SHAPES, ids=[f"n{n}-N{N}" for n, N in SHAPES])
def test_random_graphs(af, qgtc, n, N):
    src, dst = _random_graph(n, 100 + n)
    adj = qgtc.pack_edges_tiled(_dev(src), _dev(dst), n)
    for transposed in (False, True):
        _check_view(af, qgtc, adj, src, dst, n, N, transposed, f"random n={n} N={N} transposed={transposed}", bits_list=(8,) if N not in (5, 64) else (4, 8))


@pytest.mark.parametrize("n,N", [(1, 5), (33, 64), (300, 5), (300, 257)])
def test_a_graph_without_edges(af, qgtc, n, N):
    src = dst = np.zeros(0, np.int64)
    adj = qgtc.pack_edges_tiled(_dev(src), _dev(dst), n)
    assert adj.n_tiles == 0
    for transposed in (False, True):
        _check_view(af, qgtc, adj, src, dst, n, N, transposed, f"no edges n={n} N={N} transposed={transposed}", bits_list=(8,))


@pytest.mark.parametrize("N", [5, 64, 129, 257])
def test_the_degree_ladder(af, qgtc, N):
    n = 300
    for transposed in (False, True):
        src, dst = _ladder_graph(n, transposed)
        A = am.dense_view(src, dst, n, transposed)
        assert A.sum(axis=1)[:len(LADDER)].tolist() == list(LADDER) and A.sum() == sum(LADDER)
        adj = qgtc.pack_edges_tiled(_dev(src), _dev(dst), n)
        _check_view(af, qgtc, adj, src, dst, n, N, transposed, f"ladder N={N} transposed={transposed}", bits_list=(8,))


@pytest.mark.parametrize("N", [5, 64])
def test_the_hub(af, qgtc, N):
    """Node 0 of 700 is adjacent to every node and every node to it, all codes 255: the hub's sum 700 * 255 = 178 500 passes 2^16 and its
    degree 2 * 257, so a narrow partial sum that is widened too late shows; 178 500 < 2^24 keeps the planes route exact."""
    import torch

    n = 700
    src, dst = _hub_graph(n)
    adj = qgtc.pack_edges_tiled(_dev(src), _dev(dst), n)
    T = np.full((n, N), 2.5, F32)
    assert (cm.codes(T, am.qparams(T, 8), 8) == 255).all()
    for transposed in (False, True):
        a = adj.T if transposed else adj
        got = af.tiledMMCodes(a, torch.full((n, N), 255, dtype=torch.uint8, device="cuda")).cpu().numpy()
        assert (got[0] == 178500).all() and (got[1:] == 255).all()      # the hub's row; every other node's one neighbour is the hub
        _check_view(af, qgtc, adj, src, dst, n, N, transposed, f"hub N={N} transposed={transposed}", bits_list=(8,), T=T)


def _fused_entry(a, Q, qt, scale, rm, sm):
    """qgtc_tiledmm_u8_affine / _t_affine through ctypes on a code matrix Q (a [n, N] view with rows PAD4(N) apart), as a float32 tensor"""
    import torch
    from qgtc_ppopp22_amd import cabi, tiled

    n, N = Q.shape
    assert Q.stride(0) == cm.pad4(N) and Q.data_ptr() % 4 == 0
    out = torch.empty((n, N), dtype=torch.float32, device="cuda")
    fn = getattr(cabi.load(), "qgtc_tiledmm_u8" + ("_t" if a.transposed else "") + "_affine")
    rc = fn(*tiled._view_args(a), Q.data_ptr(), Q.stride(0), (n - 1) * Q.stride(0) + cm.pad4(N), N, qt.data_ptr(), scale.data_ptr(), out.data_ptr(),
            out.numel(), rm.data_ptr(), sm.data_ptr(), a.mask_words, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    return out


# ---- 3. the masks ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [5, 64])
def test_all_ones_masks_are_no_masks(af, qgtc, N):
    import torch

    n = 300
    src, dst = _random_graph(n, 21)
    adj = qgtc.pack_edges_tiled(_dev(src), _dev(dst), n)
    T = _dev(_features(n, N, 22))
    ones = _bm(np.ones(n, bool), n)
    qt = af.qparams(T, 8)
    Q = af.codes(T, 8, qt)
    for a in (adj, adj.T):
        for kw in ({"row_mask": ones, "nbr_mask": ones}, {"row_mask": ones}, {"nbr_mask": ones}):
            assert torch.equal(af.tiledMMCodes(a, Q, **kw), af.tiledMMCodes(a, Q))
            dm.same_bits(_cpu([af.aggregate(a, T, 8, route="bytes", **kw)]), _cpu([af.aggregate(a, T, 8, route="bytes")]), "all-ones masks")


@pytest.mark.parametrize("N", [5, 64, 130])
def test_dead_blocks_and_dead_neighbours_are_never_read(af, qgtc, N):
    """Wrong VALUES where the contract says nothing is read, never a wrong index (the construction of tests/test_tiled_bit_nodes_gpu.py):
    the tiles of dead blocks (32 rows on adj, a k-quad's 128 on adj.T) are overwritten with all-ones words and the code bytes of every
    neighbour outside nbr_mask with other bytes. Every index entry stays as it is. The masked outputs do not change."""
    import torch

    n = 1000
    rng = np.random.default_rng(N)
    src, dst = random_edges(rng, n, 4 * n)
    src = np.concatenate([src, rng.integers(0, n, size=4 * n, dtype=np.int64)])
    dst = np.concatenate([dst, rng.integers(0, n, size=4 * n, dtype=np.int64)])
    quad = np.arange(n) // 128
    R = np.isin(quad, (1, 4, 6)) & (rng.random(n) < 0.5)       # whole k-quads (so whole row blocks) without a live row
    S = np.isin(quad, (0, 2, 5)) & (rng.random(n) < 0.5)
    adj = qgtc.pack_edges_tiled(_dev(src), _dev(dst), n)
    T = _dev(_features(n, N, 31))
    qt = af.qparams(T, 8)
    Q = af.codes(T, 8, qt)
    scale = _dev(rng.uniform(0.5, 2.0, n).astype(F32))
    kw = {"row_mask": _bm(R, n), "nbr_mask": _bm(S, n)}
    row_ptr, kquad = adj.row_ptr.cpu().numpy(), adj.kquad.cpu().numpy()
    tile_rb = np.repeat(np.arange(row_ptr.size - 1), np.diff(row_ptr))
    Q2 = Q.as_strided((n, cm.pad4(N)), (cm.pad4(N), 1)).clone()[:, :N]       # a code matrix of its own, rows PAD4(N) apart
    Q2[_dev(np.flatnonzero(~S))] = _dev(rng.integers(0, 256, size=(int((~S).sum()), N)).astype(np.uint8))
    for transposed in (False, True):
        a = adj.T if transposed else adj
        dead_tiles = ~np.isin(kquad, (1, 4, 6)) if transposed else ~np.isin(tile_rb // 4, (1, 4, 6))
        assert dead_tiles.any() and not dead_tiles.all()
        tiles = adj.tiles.clone()
        tiles.view(-1, 128)[_dev(np.flatnonzero(dead_tiles))] = -1
        bad = qgtc.TiledAdjacency(n, adj.row_ptr, adj.kquad, tiles)
        b = bad.T if transposed else bad
        assert not torch.equal(af.tiledMMCodes(b, Q2), af.tiledMMCodes(a, Q)), "the overwritten values matter unmasked"
        assert torch.equal(af.tiledMMCodes(b, Q2, **kw), af.tiledMMCodes(a, Q, **kw)), f"transposed={transposed}"
        outs = [_fused_entry(view, codes, qt, scale, kw["row_mask"], kw["nbr_mask"]) for view, codes in ((a, Q), (b, Q2))]
        dm.same_bits(_cpu(outs[1:]), _cpu(outs[:1]), f"fused entry transposed={transposed}")


@pytest.mark.parametrize("N", [5, 64])
def test_a_non_finite_row_scale_on_a_masked_out_row(af, qgtc, N):
    """0 * NaN and 0 * inf: a row outside row_mask passes through the epilogue with acc = cnt = 0, as on the planes route."""
    n = 300
    src, dst = _random_graph(n, 41)
    adj = qgtc.pack_edges_tiled(_dev(src), _dev(dst), n)
    rng = np.random.default_rng(42)
    T = _features(n, N, 43)
    R, S = rng.random(n) < 0.5, rng.random(n) < 0.5
    scale = rng.uniform(0.5, 2.0, n).astype(F32)
    out = np.flatnonzero(~R)
    scale[out[0::3]], scale[out[1::3]], scale[out[2::3]] = np.nan, np.inf, -np.inf
    kw = {"row_mask": _bm(R, n), "nbr_mask": _bm(S, n)}
    for transposed in (False, True):
        a = adj.T if transposed else adj
        A = am.dense_view(src, dst, n, transposed)
        y = _cpu([af.aggregate(a, _dev(T), 8, _dev(scale), route="bytes", **kw)])
        assert np.isnan(y[0].numpy()[~R]).all()
        dm.same_as_model(y, [cm.aggregate(A, T, 8, scale, R, S)], "non-finite row_scale against the model")
        dm.same_bits(y, _cpu([af.aggregate(a, _dev(T), 8, _dev(scale), route="planes", **kw)]), "non-finite row_scale against planes")


# ---- 4. the C entries, called directly ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [5, 130])
def test_the_product_entries_write_their_outputs_and_nothing_else(af, qgtc, N):
    """The four product entries through ctypes, ld = PAD4(N) + 8 with other bytes from column N up to ld, into poisoned outputs with
    canaries around them, from hand-made bitmaps."""
    import torch
    from qgtc_ppopp22_amd import cabi, tiled

    n, bits = 300, 8
    lib = cabi.load()
    src, dst = _random_graph(n, 51)
    adj = qgtc.pack_edges_tiled(_dev(src), _dev(dst), n)
    rng = np.random.default_rng(52)
    T = _features(n, N, 53)
    qt = am.qparams(T, bits)
    Q = cm.codes(T, qt, bits)
    ld = cm.pad4(N) + 8
    buf = rng.integers(0, 256, size=(n, ld)).astype(np.uint8)
    buf[:, :N] = Q
    dbuf, dqt = _dev(buf), _dev(qt)
    R, S = rng.random(n) < 0.5, rng.random(n) < 0.5
    scale = rng.uniform(0.5, 2.0, n).astype(F32)
    dscale = _dev(scale)
    rm, sm = _dev(nm.bitmap(R).view(np.int32)), _dev(nm.bitmap(S).view(np.int32))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for transposed in (False, True):
        a = adj.T if transposed else adj
        A = am.dense_view(src, dst, n, transposed)
        for masks, (pr, ps, fr, fs) in (("none", (None, None, None, None)), ("both", (rm.data_ptr(), sm.data_ptr(), R, S))):
            tail = (pr, ps, adj.mask_words if pr else 0)
            for affine in (False, True):
                out = torch.full((CANARY + n * N + CANARY,), 0x7FC00000, dtype=torch.int32, device="cuda")
                fn = getattr(lib, "qgtc_tiledmm_u8" + ("_t" if transposed else "") + ("_affine" if affine else ""))
                mid = (dqt.data_ptr(), dscale.data_ptr()) if affine else ()
                rc = fn(*tiled._view_args(a), dbuf.data_ptr(), ld, n * ld, N, *mid, out.data_ptr() + 4 * CANARY, n * N, *tail, stream)
                assert rc == 0
                got = out.cpu()
                assert (got[:CANARY] == 0x7FC00000).all() and (got[CANARY + n * N:] == 0x7FC00000).all(), "a canary was overwritten"
                body = got[CANARY:CANARY + n * N].reshape(n, N)
                what = f"C entry transposed={transposed} masks={masks} affine={affine}"
                if affine:
                    dm.same_as_model([body.view(torch.float32)], [cm.fused(A, Q, qt, scale, fr, fs)], what)
                else:
                    dm.same_as_model([body], [cm.tiled_mm_codes(A, Q, fr, fs)], what)


# ---- 5. the Python surface ------------------------------------------------------------------------------------------------------------------
def test_misaligned_codes_get_a_padded_copy(af, qgtc):
    import torch

    n, N = 300, 7
    src, dst = _random_graph(n, 61)
    adj = qgtc.pack_edges_tiled(_dev(src), _dev(dst), n)
    Qn = np.random.default_rng(62).integers(0, 256, size=(n, N)).astype(np.uint8)
    A = am.dense_view(src, dst, n)
    want = [cm.tiled_mm_codes(A, Qn)]
    contiguous = _dev(Qn)                                   # row stride 7: off the 4-byte rule
    wide, fine = (torch.full((n, 16), 0xEE, dtype=torch.uint8, device="cuda") for _ in range(2))
    wide[:, 1:1 + N] = contiguous
    fine[:, 4:4 + N] = contiguous
    for Q in (contiguous, wide[:, 1:1 + N], fine[:, 4:4 + N]):     # a bad stride, a bad base, neither (other bytes behind column N)
        dm.same_as_model(_cpu([af.tiledMMCodes(adj, Q)]), want, "tiledMMCodes on a view")
    one = torch.full((1, 5), 9, dtype=torch.uint8, device="cuda")                   # a single row whose storage ends at byte 5
    adj1 = qgtc.pack_edges_tiled(_dev(np.zeros(1, np.int64)), _dev(np.zeros(1, np.int64)), 1)
    assert af.tiledMMCodes(adj1, one).tolist() == [[9] * 5]


def test_the_python_refusals(af, qgtc):
    import torch

    n, N = 40, 6
    src, dst = _random_graph(n, 71)
    adj = qgtc.pack_edges_tiled(_dev(src), _dev(dst), n)
    Q = torch.zeros((n, N), dtype=torch.uint8, device="cuda")
    T = torch.zeros((n, N), dtype=torch.float32, device="cuda")
    qp = af.qparams(T, 8)
    with pytest.raises(TypeError):
        af.tiledMMCodes(adj, Q.to(torch.int32))
    with pytest.raises(TypeError):
        af.tiledMMCodes(adj, Q.cpu().numpy())
    with pytest.raises(TypeError):
        af.tiledMMCodes("adj", Q)
    with pytest.raises(ValueError):
        af.tiledMMCodes(adj, Q.cpu())
    with pytest.raises(ValueError):
        af.tiledMMCodes(adj, Q[0])
    with pytest.raises(ValueError):
        af.tiledMMCodes(adj, Q[:n - 1])
    with pytest.raises(ValueError):
        af.tiledMMCodes(adj, Q[:, :0])
    with pytest.raises(ValueError):
        af.tiledMMCodes(adj, torch.zeros((N, n), dtype=torch.uint8, device="cuda").t())      # column stride n
    with pytest.raises(TypeError):
        af.tiledMMCodes(adj, Q, row_mask=torch.zeros(adj.mask_words, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        af.tiledMMCodes(adj, Q, nbr_mask=torch.zeros(adj.mask_words + 1, dtype=torch.int32, device="cuda"))
    with pytest.raises(TypeError):
        af.codes(T.double(), 8, qp)
    with pytest.raises(ValueError):
        af.codes(T, 9, qp)
    with pytest.raises(ValueError):
        af.codes(T, 8, torch.zeros((2, 4), device="cuda"))
    for route in ("byte", "", None, 8):
        with pytest.raises(ValueError):
            af.aggregate(adj, T, 8, route=route)
        with pytest.raises(ValueError):
            af.GCNConv_Affine(4, 4, 4, route=route)
    with pytest.raises(TypeError):
        af.aggregate(adj, T, 8, route="bytes", row_mask=torch.zeros(adj.mask_words, dtype=torch.int64, device="cuda"))
    layer = af.GCNConv_Affine(N, 4, 3, route="bytes").cuda()
    layer.route = "bits"
    with pytest.raises(ValueError):
        layer(adj, T)
    assert set(af.__all__) >= {"codes", "tiledMMCodes", "aggregate", "GCNConv_Affine"}


# ---- 6. the layer ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", [None, "mean", "sym"])
def test_the_layer_on_the_bytes_route(af, qgtc, norm):
    import torch
    from qgtc_ppopp22_amd import conv

    n, dims = 300, (12, 20, 7)
    src, dst = _random_graph(n, 81)
    A = am.dense_view(src, dst, n)
    adj = qgtc.pack_edges_tiled(_dev(src), _dev(dst), n, reorder=True)
    rng = np.random.default_rng(82)
    X, W_in, W_out = (rng.normal(size=s).astype(F32) for s in ((n, dims[0]), (dims[0], dims[1]), (dims[1], dims[2])))
    nodes = rng.random(n) < 0.6
    layers = {}
    for route in ("planes", "bytes"):
        layer = af.GCNConv_Affine(*dims, w_bit=4, act_bit=8, norm=norm, route=route).cuda()
        with torch.no_grad():
            layer.W_in.copy_(_dev(W_in))
            layer.W_out.copy_(_dev(W_out))
        layers[route] = layer
    got = {r: _cpu([l(adj, _dev(X)), l(adj, _dev(X), nodes=_dev(nodes))]) for r, l in layers.items()}
    dm.same_as_model(got["bytes"], [am.gcn(A, X, W_in, W_out, 4, 8, norm), am.gcn(A, X, W_in, W_out, 4, 8, norm, nodes)], f"layer norm={norm}")
    dm.same_bits(got["bytes"], got["planes"], f"layer bytes against planes norm={norm}")
    if norm != "mean":
        return
    fl = conv.GCNConv(*dims, norm=norm).cuda()
    with torch.no_grad():
        fl.W_in.copy_(_dev(W_in))
        fl.W_out.copy_(_dev(W_out))
    twin = af.GCNConv_Affine.from_float(fl, 4, 8, route="bytes")
    assert twin.route == "bytes" and af.GCNConv_Affine.from_float(fl).route == "planes"
    dm.same_bits(_cpu([twin(adj, _dev(X))]), got["bytes"][:1], "from_float(route='bytes')")
