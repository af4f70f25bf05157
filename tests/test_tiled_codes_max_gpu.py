"""Max and min aggregation on byte codes on the device (``affine.tiledMaxCodes``, ``affine.aggregate(reduce=)``,
``affine.GCNConv_Affine(aggr=)`` and the four C entries of include/qgtc_codes_max.h) against an inline NumPy extremum of int64 codes
over the dense masked view; dequantisation and requantisation are tests/affine_model.py's and tests/tiled_codes_model.py's. Every check
is bit for bit. Both views throughout."""
import ctypes

import numpy as np
import pytest

import affine_model as am
import dirty_memory as dm
import tiled_codes_model as cm
from test_tiled_codes_gpu import LADDER, _bm, _cpu, _dev, _hub_graph, _ladder_graph, _random_graph, af  # noqa: F401

pytestmark = pytest.mark.gpu
F32 = np.float32
n0 = 300
SHAPES = [(n0, N) for N in (1, 3, 4, 5, 64, 65, 128, 129, 256, 257, 300)] + [(n, N) for n in (1, 31, 32, 33, 127, 128, 129) for N in (5, 64)]
REDUCES = ("max", "min")


def _ext(A, Q, reduce, rm=None, sm=None):
    """(int64 [n, N] extremum of the code rows over the live neighbours - the identity where there is none -, bool [n] had a term)"""
    live = am.masked_view(A, rm, sm).astype(bool)
    full = np.where(live[:, :, None], np.asarray(Q, np.int64)[None], 0 if reduce == "max" else 255)
    return (full.max(1) if reduce == "max" else full.min(1)), live.any(1)


def _raw(A, Q, reduce, empty, rm=None, sm=None):
    m, had = _ext(A, Q, reduce, rm, sm)
    return np.where(had[:, None], m, empty).astype(np.uint8)


def _float(A, Q, qt, reduce, rm=None, sm=None):
    """scale * (m - z), +0 in a row without a term: am.dequant with the flag as the row sum of a one-term product"""
    m, had = _ext(A, Q, reduce, rm, sm)
    return am.dequant((m * had[:, None]).astype(F32), 1, am.IDENTITY, had.astype(np.int64), qt, None)


def _codes(n, N, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(n, N)).astype(np.uint8)


def _padded(Q, fill):
    """Q on the device as a view of a buffer whose bytes from column N on (pad bytes included) hold ``fill``"""
    buf = np.full((Q.shape[0], cm.pad4(Q.shape[1]) + 4), fill, np.uint8)
    buf[:, :Q.shape[1]] = Q
    return _dev(buf)[:, :Q.shape[1]]


def _views(qgtc, src, dst, n, **kw):
    adj = qgtc.pack_edges_tiled(_dev(src), _dev(dst), n, **kw)
    return [(t, adj.T if t else adj, am.dense_view(src, dst, n, t)) for t in (False, True)]


# ---- 1. raw codes: shapes and pad bytes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,N", SHAPES, ids=[f"n{n}-N{N}" for n, N in SHAPES])
def test_shapes_and_pad_bytes(af, qgtc, n, N):
    import torch
    from qgtc_ppopp22_amd import cabi, tiled

    src, dst = _random_graph(n, 100 + n)
    Q = _codes(n, N, n + N)
    ldo, lib = cm.pad4(N) + 8, cabi.load()
    for t, a, A in _views(qgtc, src, dst, n):
        for reduce in REDUCES:
            dQ = _padded(Q, 0xFF if reduce == "max" else 0x00)      # a surplus byte that leaked would win
            want = _raw(A, Q, reduce, 7)
            got = af.tiledMaxCodes(a, dQ, reduce, 7)
            assert got.dtype == torch.uint8 and tuple(got.shape) == (n, N) and got.data_ptr() % 16 == 0
            assert (got.cpu().numpy() == want).all(), f"{reduce} transposed={t}"
            out = torch.full((n, ldo), 0xA5, dtype=torch.uint8, device="cuda")
            fn = getattr(lib, "qgtc_tiledmax_u8" + ("_t" if t else ""))
            rc = fn(*tiled._view_args(a), dQ.data_ptr(), dQ.stride(0) if n > 1 else cm.pad4(N), (n - 1) * dQ.stride(0) + cm.pad4(N), N,
                    int(reduce == "min"), 7, out.data_ptr(), ldo, (n - 1) * ldo + cm.pad4(N), None, None, 0,
                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc == 0
            whole = out.cpu().numpy()
            assert (whole[:, :N] == want).all() and (whole[:, N:cm.pad4(N)] == 0).all() and (whole[:, cm.pad4(N):] == 0xA5).all()


# ---- 2. raw codes: graphs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [5, 64, 257])
@pytest.mark.parametrize("graph", ["ladder", "hub", "identity"])
def test_graphs_and_empty_rows(af, qgtc, graph, N):
    for t in (False, True):
        src, dst = _hub_graph(n0) if graph == "hub" else _ladder_graph(n0, t)
        _, a, A = _views(qgtc, src, dst, n0)[t]
        if graph == "ladder":
            assert A.sum(axis=1)[:len(LADDER)].tolist() == list(LADDER) and A.sum() == sum(LADDER)
        for reduce in REDUCES:
            # "identity": every code equals the reducer's identity, so a row with a term differs from an empty one by the flag alone
            Q = np.full((n0, N), 0 if reduce == "max" else 255, np.uint8) if graph == "identity" else _codes(n0, N, N)
            for empty in (0, 7, 255):
                got = af.tiledMaxCodes(a, _dev(Q), reduce, empty).cpu().numpy()
                assert (got == _raw(A, Q, reduce, empty)).all(), f"{graph} {reduce} empty={empty} transposed={t}"
                assert graph == "hub" or (got[len(LADDER):] == empty).all()


# ---- 3. raw codes: masks -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [5, 64])
@pytest.mark.parametrize("masks", ["half", "dead_block", "dead_quad"])
def test_masks(af, qgtc, masks, N):
    rng = np.random.default_rng(N)
    i = np.arange(n0)
    R, S = {"half": (rng.random(n0) < 0.5, rng.random(n0) < 0.5), "dead_block": (~((i >= 32) & (i < 64)), rng.random(n0) < 0.5),
            "dead_quad": (~((i >= 128) & (i < 256)), ~((i >= 128) & (i < 256)))}[masks]
    src, dst = _random_graph(n0, 21)
    Q = _codes(n0, N, 22)
    for t, a, A in _views(qgtc, src, dst, n0):
        for reduce in REDUCES:
            for rm, sm in ((R, S), (R, None), (None, S)):
                got = af.tiledMaxCodes(a, _dev(Q), reduce, 9, row_mask=_bm(rm, n0), nbr_mask=_bm(sm, n0)).cpu().numpy()
                assert (got == _raw(A, Q, reduce, 9, rm, sm)).all(), f"{masks} {reduce} transposed={t}"
                assert rm is None or (got[~rm] == 9).all()


# ---- 4. affine.aggregate(reduce=) ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reduce", REDUCES)
@pytest.mark.parametrize("bits", [1, 4, 8])
def test_aggregate_forms(af, qgtc, bits, reduce):
    n, N = n0, 37
    rng = np.random.default_rng(bits)
    T = (rng.normal(size=(n, N)) * 3.0 - 1.0).astype(F32)
    src, dst = _ladder_graph(n, False)                        # most rows are empty
    src, dst = np.concatenate([src, _random_graph(100, 3)[0]]), np.concatenate([dst, _random_graph(100, 3)[1]])
    R, S = rng.random(n) < 0.7, rng.random(n) < 0.7
    qt = am.qparams(T, bits)
    Q, z = cm.codes(T, qt, bits), int(qt[0, 1])
    other = am.qparams(T * F32(0.5), 4)
    dT, dqt, dother = _dev(T), _dev(qt), _dev(other)
    for t, a, A in _views(qgtc, src, dst, n):
        for rm, sm in ((None, None), (R, S)):
            kw = {"row_mask": _bm(rm, n), "nbr_mask": _bm(sm, n)}
            want = _float(A, Q, qt, reduce, rm, sm)
            y = af.aggregate(a, dT, bits, route="bytes", reduce=reduce, **kw)
            dm.same_as_model(_cpu([y]), [want], f"float out {reduce} transposed={t}")
            dm.same_bits(_cpu([af.aggregate(a, _dev(Q), bits, route="bytes", t_qparams=dqt, reduce=reduce, **kw)]), _cpu([y]), "uint8 in")
            same = af.aggregate(a, dT, bits, route="bytes", t_qparams=dqt, out=(bits, dqt), reduce=reduce, **kw)
            assert (same.cpu().numpy() == _raw(A, Q, reduce, z, rm, sm)).all(), "out under the same row is the raw codes"
            assert (same.cpu().numpy() == af.tiledMaxCodes(a, _dev(Q), reduce, z, **kw).cpu().numpy()).all()
            req = af.aggregate(a, dT, bits, route="bytes", out=(4, dother), reduce=reduce, **kw)
            assert (req.cpu().numpy() == cm.codes(want, other, 4)).all(), "out under another row"
            deq = _dev(am.dequant(Q.astype(F32), 1, am.IDENTITY, np.ones(n, np.int64), qt, None))
            dm.same_bits(_cpu([y]), _cpu([qgtc.tiledMMFloat(a, deq, reduce=reduce, **kw)]), "against the float extremum of the dequantised codes")


# ---- 5. the layer ----------------------------------------------------------------------------------------------------------------------------
def _model_layer(A, X, W_in, W_out, reduce, nodes=None):
    def agg(T):
        qt = am.qparams(T, 8)
        return _float(A, cm.codes(T, qt, 8), qt, reduce, nodes, nodes)
    return agg(am.linear(agg(am.linear(X, W_in, 8, 4)), W_out, 8, 4))


@pytest.mark.parametrize("reduce", REDUCES)
def test_the_layer(af, qgtc, reduce):
    import torch
    from qgtc_ppopp22_amd import conv

    n, dims = n0, (12, 20, 7)
    src, dst = _random_graph(n, 81)
    A = am.dense_view(src, dst, n)
    adj = qgtc.pack_edges_tiled(_dev(src), _dev(dst), n, reorder=True)
    rng = np.random.default_rng(82)
    X, W_in, W_out = (rng.normal(size=s).astype(F32) for s in ((n, dims[0]), (dims[0], dims[1]), (dims[1], dims[2])))
    nodes = rng.random(n) < 0.6
    fl = conv.GCNConv(*dims, aggr=reduce).cuda()
    with torch.no_grad():
        fl.W_in.copy_(_dev(W_in))
        fl.W_out.copy_(_dev(W_out))
    layer = af.GCNConv_Affine.from_float(fl, 4, 8, route="bytes", linear_route="bytes")
    assert layer.aggr == reduce
    dX, dn = _dev(X), _dev(nodes)
    got = _cpu([layer(adj, dX), layer(adj, dX, nodes=dn)])
    dm.same_as_model(got, [_model_layer(A, X, W_in, W_out, reduce), _model_layer(A, X, W_in, W_out, reduce, nodes)], f"layer aggr={reduce}")
    static = [layer(adj, dX, act_qparams=layer.calibrate(adj, dX)), layer(adj, dX, nodes=dn, act_qparams=layer.calibrate(adj, dX, nodes=dn))]
    dm.same_bits(_cpu(static), got, f"static chain aggr={reduce}")


def test_the_refusals(af, qgtc):
    import torch
    from qgtc_ppopp22_amd import cabi, tiled

    n, N = 40, 6
    src, dst = _random_graph(n, 71)
    adj = qgtc.pack_edges_tiled(_dev(src), _dev(dst), n)
    T = torch.ones((n, N), dtype=torch.float32, device="cuda")
    Q = torch.zeros((n, N), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match='route="bytes"'):
        af.aggregate(adj, T, 8, reduce="max")
    with pytest.raises(ValueError, match='row_scale cannot be combined with reduce="min"'):
        af.aggregate(adj, T, 8, adj.mean_scale(), route="bytes", reduce="min")
    with pytest.raises(ValueError, match="reduce"):
        af.aggregate(adj, T, 8, route="bytes", reduce="mean")
    with pytest.raises(ValueError, match="norm"):
        af.GCNConv_Affine(N, 4, 3, norm="mean", route="bytes", aggr="max")
    with pytest.raises(ValueError, match='route="bytes"'):
        af.GCNConv_Affine(N, 4, 3, aggr="max")
    layer = af.GCNConv_Affine(N, 4, 3, route="bytes", linear_route="bytes", aggr="max").cuda()
    with pytest.raises(ValueError, match="fuse=False"):
        layer(adj, T, act_qparams=layer.calibrate(adj, T), fuse=True)
    for empty in (256, -1):
        with pytest.raises(ValueError, match="empty"):
            af.tiledMaxCodes(adj, Q, "max", empty)
    out = torch.zeros((n, 8), dtype=torch.uint8, device="cuda")
    rc = cabi.load().qgtc_tiledmax_u8(*tiled._view_args(adj), Q.data_ptr(), 8, n * 8, N, 0, 256, out.data_ptr(), 8, n * 8, None, None, 0, None)
    assert rc == 1                                            # QGTC_EINVAL, before any device work
    assert "tiledMaxCodes" in af.__all__


# ---- 6. graph capture ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reduce", REDUCES)
def test_replays_of_a_captured_aggregate(af, qgtc, reduce):
    import torch

    n, N = n0, 70
    src, dst = _random_graph(n, 91)
    adj = qgtc.pack_edges_tiled(_dev(src), _dev(dst), n)
    rng = np.random.default_rng(92)
    inputs = [_dev(rng.normal(size=(n, N)).astype(F32) * F32(k + 1)) for k in range(3)]
    eager = [[af.aggregate(a, x, 8, route="bytes", reduce=reduce).cpu() for a in (adj, adj.T)] for x in inputs]
    side, x = torch.cuda.Stream(), inputs[0].clone()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ys = [af.aggregate(a, x, 8, route="bytes", reduce=reduce) for a in (adj, adj.T)]
    for k in (1, 2, 0, 2):
        x.copy_(inputs[k])
        graph.replay()
        torch.cuda.synchronize()
        dm.same_bits(_cpu(ys), eager[k], f"replay of input {k}")
