"""The extremum tiled products on the device (QGTC.tiledMMFloat(reduce="max" | "min"), QGTC.tiledAggregate(reduce=), conv.GCNConv(aggr=)
and the four C-ABI entries behind them) against the exact model of tests/tiled_max_model.py. The forward moves words and the select adds
in a fixed order, so every float comparison is bit for bit (a NaN equals a NaN), every `arg` comparison is integer equality, nothing is
sampled and no tolerance is used."""
import ctypes

import numpy as np
import pytest

from stream_cases import Live, capture_and_replay, eager_results, empty, env_of, ordering_probe, warm_adjacency
from test_tiled_float_gpu import CANARY, NAN_WORD, NO_EDGES, SWEEP, assert_floats_identical
from tiled_float_model import neighbour_lists
from tiled_max_model import (MAX, MAX_FORWARD_VARIANTS, MAX_TRANSPOSED_VARIANTS, MIN, SELECT_FORWARD_VARIANTS, SELECT_TRANSPOSED_VARIANTS,
                             extremum_f32, max_chunks, max_variant, select_f32)
from tiled_model import random_edges, set_cells

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A                              # what `arg` holds before a C entry writes it
OPS = ((MAX, "max"), (MIN, "min"))


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def lib():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    from qgtc_ppopp22_amd import cabi

    return cabi.load()


def _index(adj, transposed, null=False):
    if null:
        return (None,) * (4 if transposed else 3)
    if transposed:
        t = adj.T
        return _ptr(t.col_ptr), _ptr(t.col_tile), _ptr(t.col_rb), _ptr(adj.tiles)
    return _ptr(adj.row_ptr), _ptr(adj.kquad), _ptr(adj.tiles)


def _raw_max(torch, lib, adj, X, op, transposed, with_arg=True, null_index=False):
    """The C forward entry on `out` pre-filled with NaN and `arg` with SENTINEL, each followed by CANARY words:
    (out [n, N], arg [n, N] or None). The canaries are checked here."""
    n, N = X.shape
    out = torch.full((n * N + CANARY,), float("nan"), dtype=torch.float32, device="cuda")
    arg = torch.full((n * N + CANARY,), SENTINEL, dtype=torch.int32, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    entry = lib.qgtc_tiledmax_f32_t if transposed else lib.qgtc_tiledmax_f32
    rc = entry(*_index(adj, transposed, null_index), 0 if null_index else adj.n_tiles, n, X.data_ptr(), X.numel(), N, op, out.data_ptr(),
               n * N, arg.data_ptr() if with_arg else None, n * N if with_arg else 0, st)
    assert rc == 0, rc
    o, a = out.cpu().numpy(), arg.cpu().numpy()
    assert (o[n * N:].view(np.uint32) == NAN_WORD).all(), "canaries after out"
    assert (a[n * N:] == SENTINEL).all(), "canaries after arg"
    if not with_arg:
        assert (a == SENTINEL).all(), "arg is NULL: nothing may be written"
        return o[: n * N].reshape(n, N), None
    return o[: n * N].reshape(n, N), a[: n * N].reshape(n, N)


def _raw_sel(torch, lib, adj, dY, arg, transposed, null_index=False):
    n, N = dY.shape
    out = torch.full((n * N + CANARY,), float("nan"), dtype=torch.float32, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    entry = lib.qgtc_tiledsel_f32_t if transposed else lib.qgtc_tiledsel_f32
    rc = entry(*_index(adj, transposed, null_index), 0 if null_index else adj.n_tiles, n, dY.data_ptr(), dY.numel(), N, arg.data_ptr(),
               arg.numel(), out.data_ptr(), n * N, st)
    assert rc == 0, rc
    o = out.cpu().numpy()
    assert (o[n * N:].view(np.uint32) == NAN_WORD).all(), "canaries after out"
    return o[: n * N].reshape(n, N)


def _select(adj, dY, arg):
    """The select through the binding (the private wrapper QGTC.tiledAggregate's backward calls)."""
    from qgtc_ppopp22_amd.tiled import _tiled_select

    return _tiled_select(adj, dY, arg)


def assert_forward(got_out, got_arg, want_out, want_arg, X, what):
    assert_floats_identical(got_out, want_out, what)
    np.testing.assert_array_equal(got_arg, want_arg, err_msg=what + " arg")
    has = got_arg >= 0                             # the value is the winner's own word, sign bit included
    cols = np.broadcast_to(np.arange(X.shape[1]), got_arg.shape)
    assert_floats_identical(got_out[has], X[got_arg[has], cols[has]], what + " out is X[arg]")
    assert (_bits(got_out)[~has] == 0).all(), what + " a row without neighbours gives +0"


def _tied(rng, n, N):
    """Standard-normal values, half of them rounded to halves so that ties are everywhere."""
    x = rng.standard_normal((n, N)).astype(np.float32)
    return np.where(rng.random((n, N)) < 0.5, np.round(x * 2) / 2, x).astype(np.float32)


# ---- 1. the sweep: every variant, both ops, both views, both ways in, and the select --------------------------------------------------
def test_the_sweep_hits_every_variant():
    """Against tests/tiled_max_model.py's copy of the launchers' switches (tiled_max_kernels.hip.h, tiled_max_t_kernels.hip.h), not against
    the
    launchers themselves: a width changed there must be changed in the model too, or this still passes."""
    for transposed, select, variants in ((False, False, MAX_FORWARD_VARIANTS), (True, False, MAX_TRANSPOSED_VARIANTS),
                                         (False, True, SELECT_FORWARD_VARIANTS), (True, True, SELECT_TRANSPOSED_VARIANTS)):
        hit = {}
        for _, N in SWEEP:
            hit.setdefault(max_variant(N, transposed, select), set()).add(N)
        assert sorted(hit) == sorted(variants)
        assert all(len(Ns) >= 2 for Ns in hit.values()), hit       # each at a ragged N and at its full width
        assert max(max_chunks(N, transposed, select) for _, N in SWEEP) >= 2
    assert max(n for n, _ in SWEEP) == 4097 and max(N for _, N in SWEEP) == 383


@pytest.mark.parametrize("n,N", SWEEP, ids=[f"n{n}-N{N}" for n, N in SWEEP])
def test_every_variant_equals_the_model(qgtc, lib, n, N):
    import torch

    rng = np.random.default_rng(13 * n + N)
    src, dst = random_edges(rng, n, 6 * n + 5)
    X, dY = _tied(rng, n, N), rng.standard_normal((n, N)).astype(np.float32)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    dX, ddY = _dev(torch, X), _dev(torch, dY)
    for transposed in (False, True):
        a, other = (adj.T, adj) if transposed else (adj, adj.T)
        for op, name in OPS:
            want, warg = extremum_f32(src, dst, n, X, transposed, op)
            assert not np.isnan(want).any()
            empty = slice(32, 64) if (n >= 96 and not transposed) else slice(128, 256) if (n >= 512 and transposed) else None
            if empty is not None:                  # the empty row block / the empty k-quad
                assert (_bits(want[empty]) == 0).all() and (warg[empty] == -1).all()
            what = f"{'adj.T' if transposed else 'adj'} {name} variant={max_variant(N, transposed)}"
            got, garg = qgtc.tiledMMFloat(a, dX, reduce=name, return_arg=True)
            assert got.dtype == torch.float32 and got.shape == (n, N) and got.is_contiguous(), what
            assert garg.dtype == torch.int32 and garg.shape == (n, N) and garg.is_contiguous(), what
            assert_forward(got.cpu().numpy(), garg.cpu().numpy(), want, warg, X, what)
            alone = qgtc.tiledMMFloat(a, dX, reduce=name)
            assert isinstance(alone, torch.Tensor)
            assert_floats_identical(alone.cpu().numpy(), want, what + " (no arg)")
            raw, rarg = _raw_max(torch, lib, adj, dX, op, transposed)
            assert_forward(raw, rarg, want, warg, X, what + " (C entry)")
            raw, _ = _raw_max(torch, lib, adj, dX, op, transposed, with_arg=False)
            assert_floats_identical(raw, want, what + " (C entry, arg NULL)")
            # the gradient of this forward: the select on the other view with the model's arg
            wsel = select_f32(src, dst, n, dY, warg, not transposed)
            what = f"select on {'adj' if transposed else 'adj.T'} of {name} variant={max_variant(N, not transposed, True)}"
            darg = _dev(torch, warg)
            assert_floats_identical(_select(other, ddY, darg).cpu().numpy(), wsel, what)
            assert_floats_identical(_raw_sel(torch, lib, adj, ddY, darg, not transposed), wsel, what + " (C entry)")


# ---- 2. long lists --------------------------------------------------------------------------------------------------------------------
def test_long_lists_and_the_tie_rule(qgtc):
    """Node h is adjacent to all and all are adjacent to it: its row has 999 neighbours over 8 tiles (many full queues), its k-quad's
    list has 32 tiles (four transposed rounds). A constant, a strictly ascending and a strictly descending column: the winner is the
    lowest id, the highest id, the lowest id (max; mirrored for min)."""
    import torch

    n, h = 1000, 500
    others = np.delete(np.arange(n, dtype=np.int64), h)
    src = np.concatenate([np.full(n - 1, h, np.int64), others])
    dst = np.concatenate([others, np.full(n - 1, h, np.int64)])
    rng = np.random.default_rng(2)
    X = _tied(rng, n, 35)
    X[:, 0], X[:, 1], X[:, 2] = 3.0, np.arange(n), -np.arange(n, dtype=np.float32)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    t = adj.T
    assert int(adj.degrees()[h]) == n - 1 and int(t.degrees()[h]) == n - 1
    assert int((adj.row_ptr[h // 32 + 1] - adj.row_ptr[h // 32]).item()) == 8
    assert int((t.col_ptr[h // 128 + 1] - t.col_ptr[h // 128]).item()) == 32
    lo, hi = 0, n - 1
    for transposed, a in ((False, adj), (True, t)):
        for op, name in OPS:
            got, garg = qgtc.tiledMMFloat(a, _dev(torch, X), reduce=name, return_arg=True)
            got, garg = got.cpu().numpy(), garg.cpu().numpy()
            want, warg = extremum_f32(src, dst, n, X, transposed, op)
            assert_forward(got, garg, want, warg, X, f"transposed={transposed} {name}")
            assert garg[h, :3].tolist() == ([lo, hi, lo] if op == MAX else [lo, lo, hi])
            assert (garg[others] == h).all()       # every other row sees h alone


# ---- 3. special values ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,N", [(1000, 20), (4097, 70)])
def test_special_values(qgtc, n, N):
    """A planted NaN reaches exactly the rows adjacent to it and wins there; infinities are ordinary values; in a column of zeros of
    both signs the result carries the winner's sign bit."""
    import torch

    rng = np.random.default_rng(n + N)
    src, dst = random_edges(rng, n, 6 * n + 5)
    X = _tied(rng, n, N)
    nans = [(n // 2, 0), (n // 3, 1), (n - 1, N - 1), (7, 1), (8, 1)]
    for v, c in nans:
        X[v, c] = np.nan
    for v, c, val in ((5, 2, -np.inf), (40, 3, np.inf), (n // 3, 4, -np.inf), (n // 2, 4, np.inf), (n // 3, 5, np.inf)):
        X[v, c] = val
    X[:, 6] = np.where(rng.random(n) < 0.5, np.float32(-0.0), np.float32(0.0))
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    for transposed in (False, True):
        a = adj.T if transposed else adj
        out_row, nb, _ = neighbour_lists(src, dst, n, transposed)
        bad = np.zeros((n, N), bool)
        for v, c in nans:
            bad[out_row[nb == v], c] = True
        assert bad.any(axis=0).sum() >= 3
        for op, name in OPS:
            want, warg = extremum_f32(src, dst, n, X, transposed, op)
            np.testing.assert_array_equal(np.isnan(want), bad)                      # the model's NaNs: these rows and no others
            got, garg = qgtc.tiledMMFloat(a, _dev(torch, X), reduce=name, return_arg=True)
            got, garg = got.cpu().numpy(), garg.cpu().numpy()
            np.testing.assert_array_equal(np.isnan(got), bad, err_msg=f"transposed={transposed} {name}")
            assert_forward(got, garg, want, warg, X, f"transposed={transposed} {name}")
            assert np.isnan(X[garg[bad], np.nonzero(bad)[1]]).all()                 # where a NaN arrives, a NaN won
            assert np.isinf(got).any()
            zeros = _bits(got[:, 6][garg[:, 6] >= 0])
            assert (zeros == 0).any() and (zeros == 0x80000000).any()               # both signs survive: the winner's


# ---- 4. the select treats arg as data ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,N", [(97, 33), (1000, 70)])
def test_the_select_only_compares_arg(qgtc, lib, n, N):
    """arg of random int32 - -1, non-neighbours, values from n up to 2^31 - 1, large negatives - mixed with true winners; NaN and
    infinities sit in dY wherever arg names no node at all. The result equals the model and is finite."""
    import torch

    rng = np.random.default_rng(5 * n + N)
    src, dst = random_edges(rng, n, 6 * n + 5)
    X = _tied(rng, n, N)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    for transposed in (False, True):               # the view the select runs on
        a = adj.T if transposed else adj
        _, arg = extremum_f32(src, dst, n, X, not transposed, MAX)
        kind = rng.integers(0, 6, size=arg.shape)
        junk = np.select([kind == 0, kind == 1, kind == 2, kind == 3],
                         [np.full(arg.shape, -1), rng.integers(0, n, size=arg.shape), rng.integers(n, 2 ** 31, size=arg.shape),
                          rng.integers(-2 ** 31, -1, size=arg.shape)], arg).astype(np.int32)
        junk[0, 0], junk[n - 1, N - 1] = 2 ** 31 - 1, -2 ** 31
        dY = rng.standard_normal((n, N)).astype(np.float32)
        nobody = (junk < 0) | (junk >= n)
        dY[nobody] = np.array([np.nan, np.inf, -np.inf], np.float32)[rng.integers(0, 3, size=int(nobody.sum()))]
        want = select_f32(src, dst, n, dY, junk, transposed)
        assert np.isfinite(want).all() and np.count_nonzero(want) > n // 4 and nobody.mean() > 0.3
        dj, dd = _dev(torch, junk), _dev(torch, dY)
        assert_floats_identical(_select(a, dd, dj).cpu().numpy(), want, f"transposed={transposed}")
        assert_floats_identical(_raw_sel(torch, lib, adj, dd, dj, transposed), want, f"transposed={transposed} (C entry)")


# ---- 5. an adjacency without tiles ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,N", [(1, 1), (300, 24), (4097, 257)])
def test_an_empty_adjacency(qgtc, lib, n, N):
    """n_tiles = 0: +0 and -1 from the forward, +0 from the select; through the Python layer and through the C entries with NULL index
    pointers."""
    import torch

    rng = np.random.default_rng(n)
    adj = qgtc.pack_edges_tiled(_dev(torch, NO_EDGES[0]), _dev(torch, NO_EDGES[1]), n)
    assert adj.n_tiles == 0
    X = _dev(torch, rng.standard_normal((n, N)).astype(np.float32))
    arg = _dev(torch, rng.integers(-1, n, size=(n, N)).astype(np.int32))
    for transposed in (False, True):
        a = adj.T if transposed else adj
        for op, name in OPS:
            got, garg = qgtc.tiledMMFloat(a, X, reduce=name, return_arg=True)
            assert (got.cpu().numpy().view(np.uint32) == 0).all() and (garg.cpu().numpy() == -1).all(), (transposed, name)
            raw, rarg = _raw_max(torch, lib, adj, X, op, transposed, null_index=True)
            assert (raw.view(np.uint32) == 0).all() and (rarg == -1).all(), (transposed, name)
            raw, _ = _raw_max(torch, lib, adj, X, op, transposed, with_arg=False, null_index=True)
            assert (raw.view(np.uint32) == 0).all()
        assert (_select(a, X, arg).cpu().numpy().view(np.uint32) == 0).all()
        assert (_raw_sel(torch, lib, adj, X, arg, transposed, null_index=True).view(np.uint32) == 0).all()


# ---- 6. autograd --------------------------------------------------------------------------------------------------------------------------
def _views(torch, qgtc, src, dst, n):
    """(name, adjacency, transposed, the edge list in the adjacency's numbering) for adj, adj.T and a reordered adjacency."""
    dsrc, ddst = _dev(torch, src), _dev(torch, dst)
    adj, re = qgtc.pack_edges_tiled(dsrc, ddst, n), qgtc.pack_edges_tiled(dsrc, ddst, n, reorder=True)
    rank = re.rank.cpu().numpy()
    return [("adj", adj, False, src, dst), ("adj.T", adj.T, True, src, dst), ("reordered", re, False, rank[src], rank[dst]),
            ("reordered.T", re.T, True, rank[src], rank[dst])]


@pytest.mark.parametrize("n,N", [(97, 20), (1000, 70)])
def test_autograd_equals_the_select(qgtc, n, N):
    import torch

    rng = np.random.default_rng(3 * n + N)
    src, dst = random_edges(rng, n, 6 * n + 5)
    X, dY = _tied(rng, n, N), rng.standard_normal((n, N)).astype(np.float32)
    for view, a, transposed, s, d in _views(torch, qgtc, src, dst, n):
        for op, name in OPS:
            Xg = _dev(torch, X).requires_grad_(True)
            Y = qgtc.tiledAggregate(a, Xg, reduce=name)
            assert Y.requires_grad
            assert torch.equal(Y.detach().view(torch.int32), qgtc.tiledMMFloat(a, Xg.detach(), reduce=name).view(torch.int32)), (view, name)
            want, warg = extremum_f32(s, d, n, X, transposed, op)
            assert_floats_identical(Y.detach().cpu().numpy(), want, f"{view} {name}")
            Y.backward(_dev(torch, dY))
            assert_floats_identical(Xg.grad.cpu().numpy(), select_f32(s, d, n, dY, warg, not transposed), f"{view} {name} grad")
    # a non-contiguous dY is made contiguous by the backward
    a = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    Xg = _dev(torch, X).requires_grad_(True)
    wide = _dev(torch, np.repeat(dY, 2, axis=1))
    qgtc.tiledAggregate(a, Xg, reduce="max").backward(wide[:, ::2])
    _, warg = extremum_f32(src, dst, n, X, False, MAX)
    assert_floats_identical(Xg.grad.cpu().numpy(), select_f32(src, dst, n, dY, warg, True), "strided dY")


@pytest.mark.parametrize("n", [97, 300])
def test_autograd_equals_a_dense_reference(qgtc, n):
    """Tie-free X and integer-valued dY (the gradient's sums are exact in any order): forward and gradient equal torch's
    where(mask, X, -+inf).amax / amin on the dense adjacency, exactly."""
    import torch

    N = 8
    rng = np.random.default_rng(n)
    src, dst = random_edges(rng, n, 6 * n + 5)
    X = (rng.permutation(n * N).reshape(n, N) - n * N // 2).astype(np.float32)
    dY = _dev(torch, rng.integers(-8, 9, size=(n, N)).astype(np.float32))
    for view, a, transposed, s, d in _views(torch, qgtc, src, dst, n):
        cells = set_cells(s, d, n)
        A = np.zeros((n, n), bool)
        A[cells // n, cells % n] = True
        A = _dev(torch, A.T.copy() if transposed else A)
        for op, name in OPS:
            Xg, Xr = _dev(torch, X).requires_grad_(True), _dev(torch, X).requires_grad_(True)
            masked = torch.where(A[:, :, None], Xr[None, :, :], torch.full((), float("inf") if op == MIN else float("-inf"), device="cuda"))
            ref = masked.amin(dim=1) if op == MIN else masked.amax(dim=1)
            ref = torch.where(A.any(dim=1)[:, None], ref, torch.zeros((), device="cuda"))
            Y = qgtc.tiledAggregate(a, Xg, reduce=name)
            assert torch.equal(Y.detach().view(torch.int32), ref.detach().view(torch.int32)), (view, name)
            Y.backward(dY)
            ref.backward(dY)
            assert torch.equal(Xg.grad.view(torch.int32), Xr.grad.view(torch.int32)), (view, name)
            assert Xg.grad.abs().max() > 0


# ---- 7. determinism -----------------------------------------------------------------------------------------------------------------------
def test_two_launches_give_identical_bits(qgtc):
    import torch

    n, N = 4097, 96
    rng = np.random.default_rng(6)
    src, dst = random_edges(rng, n, 6 * n + 5)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    X, dY = _dev(torch, _tied(rng, n, N)), _dev(torch, rng.standard_normal((n, N)).astype(np.float32))
    for a in (adj, adj.T):
        for _, name in OPS:
            first, again = qgtc.tiledMMFloat(a, X, reduce=name, return_arg=True), qgtc.tiledMMFloat(a, X, reduce=name, return_arg=True)
            assert torch.equal(first[0].view(torch.int32), again[0].view(torch.int32)) and torch.equal(first[1], again[1]), a.transposed
            g1, g2 = _select(a.T, dY, first[1]), _select(a.T, dY, first[1])
            assert torch.equal(g1.view(torch.int32), g2.view(torch.int32)), a.transposed
            assert int(torch.count_nonzero(g1)) > n


# ---- 8. streams and graph capture ---------------------------------------------------------------------------------------------------------
def _live(env, transposed, name):
    """Forward and backward as a ``Live`` case of tests/stream_cases.py; the reference is the eager result on the default stream."""
    torch = env.torch
    n, N = 600, 40
    rng = np.random.default_rng(41)
    src, dst = random_edges(rng, n, 6 * n + 5)
    adj = warm_adjacency(env, src, dst, n)
    a = adj.T if transposed else adj
    data = [(_tied(rng, n, N), rng.standard_normal((n, N)).astype(np.float32)) for _ in range(4)]      # (X, dY)
    X, dY = bufs = [empty(env, (n, N), torch.float32).requires_grad_(True), empty(env, (n, N), torch.float32)]

    def run():
        Y = env.Q.tiledAggregate(a, X, reduce=name)
        return [Y.detach(), torch.autograd.grad(Y, X, dY)[0]]

    return Live(torch, bufs, data, eager_results(torch, bufs, data, run), run=run, keep=adj)


@pytest.mark.parametrize("name", ["max", "min"])
@pytest.mark.parametrize("transposed", [False, True], ids=["adj", "adjT"])
def test_side_stream_and_graph_capture(qgtc, oracle, transposed, name):
    """Forward and backward behind a timed head start on three fresh side streams (``ordering_probe``) and captured into a graph; three
    replays on new inputs equal the eager results (``capture_and_replay``)."""
    import torch

    live = _live(env_of(qgtc, oracle, torch), transposed, name)
    what = f"{name}, {'adj.T' if transposed else 'adj'}"
    ordering_probe(torch, qgtc, live, what)
    capture_and_replay(torch, qgtc, live, what)


# ---- 9. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals(qgtc):
    import torch

    from qgtc_ppopp22_amd.conv import GCNConv

    n, N = 100, 8
    src, dst = random_edges(np.random.default_rng(8), n, 6 * n)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n)
    good = torch.ones(n, N, dtype=torch.float32, device="cuda")
    scale = torch.ones(n, dtype=torch.float32, device="cuda")
    for a in (adj, adj.T):
        for fn in (qgtc.tiledMMFloat, qgtc.tiledAggregate):
            for bad in ("mean", "MAX", None, 0):
                with pytest.raises(ValueError, match="reduce"):
                    fn(a, good, reduce=bad)
            for name in ("max", "min"):
                with pytest.raises(ValueError, match="row_scale"):
                    fn(a, good, row_scale=scale, reduce=name)
                with pytest.raises(ValueError, match="src_scale"):
                    fn(a, good, src_scale=scale, reduce=name)
        with pytest.raises(ValueError, match="return_arg"):
            qgtc.tiledMMFloat(a, good, return_arg=True)
        with pytest.raises(ValueError, match="return_arg"):
            qgtc.tiledMMFloat(a, good, scale, reduce="sum", return_arg=True)
        for name in ("max", "min"):                # the operand refusals are the sum's
            with pytest.raises(TypeError, match="float16"):
                qgtc.tiledMMFloat(a, good.half(), reduce=name)
            with pytest.raises(TypeError, match="float64"):
                qgtc.tiledAggregate(a, good.double(), reduce=name)
            with pytest.raises(ValueError, match=rf"\[{n - 1}, {N}\]"):
                qgtc.tiledMMFloat(a, good[:-1].contiguous(), reduce=name)
            with pytest.raises(ValueError, match="strides"):
                qgtc.tiledMMFloat(a, torch.ones(N, n, dtype=torch.float32, device="cuda").t(), reduce=name)
            with pytest.raises(ValueError, match="cpu"):
                qgtc.tiledMMFloat(a, good.cpu(), reduce=name, return_arg=True)
    with pytest.raises(TypeError, match="TiledAdjacency"):
        qgtc.tiledMMFloat((adj.row_ptr, adj.kquad, adj.tiles), good, reduce="max")
    # the binding's keyword overload: the select has no winners to return, the forward takes no arg
    from qgtc_ppopp22_amd.tiled import _ext

    arg = torch.zeros(n, N, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="return_arg"):
        _ext._tiled_mm_f32(adj.row_ptr, adj.kquad, adj.tiles, n, good, reduce="select", arg=arg, return_arg=True)
    with pytest.raises(RuntimeError, match="arg"):
        _ext._tiled_mm_f32(adj.row_ptr, adj.kquad, adj.tiles, n, good, reduce="max", arg=arg)
    # no second derivative: differentiating the backward raises instead of giving zeros
    Xg = good.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(qgtc.tiledAggregate(adj, Xg, reduce="max").square().sum(), Xg, create_graph=True)   # dY = 2 Y has a graph
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()
    # defaults give exactly the call that was
    assert torch.equal(qgtc.tiledMMFloat(adj, good, reduce="sum"), qgtc.tiledMMFloat(adj, good))
    assert torch.equal(qgtc.tiledAggregate(adj, good, scale, reduce="sum"), qgtc.tiledMMFloat(adj, good, scale))
    # the layer
    with pytest.raises(ValueError, match="aggr"):
        GCNConv(8, 8, 4, aggr="mean")
    for norm in ("mean", "sym"):
        with pytest.raises(ValueError, match="norm"):
            GCNConv(8, 8, 4, norm=norm, aggr="max")
    assert GCNConv(8, 8, 4).aggr == "sum" and GCNConv(8, 8, 4, norm="sym").aggr == "sum"
    m = GCNConv(N, 8, 4, aggr="min").cuda()
    with pytest.raises(NotImplementedError, match="aggr"):
        m(torch.zeros(n, n, device="cuda"), good)
    assert m(adj, good).shape == (n, 4)


# ---- 10. the layer ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aggr", ["max", "min"])
def test_gcnconv_equals_the_composition(qgtc, aggr):
    import torch

    from qgtc_ppopp22_amd.conv import GCNConv

    n = 1213
    torch.manual_seed(0)
    src, dst = random_edges(np.random.default_rng(n), n, 8 * n)
    adj = qgtc.pack_edges_tiled(_dev(torch, src), _dev(torch, dst), n, reorder=True)
    assert adj.perm is not None and (adj.perm.cpu().numpy() != np.arange(n)).any()
    X = torch.randn(n, 48, device="cuda")
    target = torch.randint(0, 10, (n,), device="cuda")
    m = GCNConv(48, 64, 10, aggr=aggr).cuda()
    with torch.no_grad():
        m.W_in.mul_(0.2)
        m.W_out.mul_(0.2)
    for a in (adj, adj.T):
        agg = lambda x: qgtc.tiledMMFloat(a, x, reduce=aggr)       # noqa: E731
        with torch.no_grad():
            want = a.to_old(agg(torch.mm(agg(torch.mm(a.to_new(X), m.W_in)), m.W_out)))
            got = m(a, X)
        assert got.shape == (n, 10) and torch.equal(got.view(torch.int32), want.view(torch.int32)), a.transposed
        # one SGD step: the gradients are those of the same composition built from tiledAggregate
        opt = torch.optim.SGD(m.parameters(), lr=0.1)
        opt.zero_grad(set_to_none=True)
        torch.nn.functional.cross_entropy(m(a, X), target).backward()
        W_in, W_out = m.W_in.detach().clone().requires_grad_(True), m.W_out.detach().clone().requires_grad_(True)
        diff = lambda x: qgtc.tiledAggregate(a, x, reduce=aggr)    # noqa: E731
        torch.nn.functional.cross_entropy(a.to_old(diff(torch.mm(diff(torch.mm(a.to_new(X), W_in)), W_out))), target).backward()
        for name, p, w in (("W_in", m.W_in, W_in), ("W_out", m.W_out, W_out)):
            assert torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, name
            assert torch.equal(p.grad.view(torch.int32), w.grad.view(torch.int32)), name
        before = m.W_in.detach().clone()
        opt.step()
        assert not torch.equal(m.W_in.detach(), before)
