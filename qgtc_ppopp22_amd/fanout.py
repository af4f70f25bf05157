"""Fixed-fanout neighbour sampling on the tiled adjacency (include/qgtc_fanout.h): at most ``k`` neighbours per
node, drawn inside the tile walk, so that GraphSAGE-style training needs no second adjacency per step.

:func:`sample_fanout` takes a sample on one view of an adjacency - one selection launch gives ``thr`` uint32 [n], the k-th largest cell
hash of every node of that view (0 where the node has at most k cells) - and returns a :class:`FanoutSample`. ``fanout=`` of
``tiled.tiledMMFloat`` / ``tiled.tiledAggregate`` takes such a sample, or a pair ``(k, seed)`` from which it takes one on the view passed.
On the view it was taken on a sample is used in the OWN form (the thresholds are the output rows'), on the other view in the NBR form (the
thresholds are the neighbours'): the same kept cells either way, which is what a backward needs.

This module holds the ctypes calls of the ten entries and every allocation of the feature; ``tiled.py`` delegates to it. All launches go
to ``torch.cuda.current_stream()`` and read nothing back, so they can be captured into a graph (a captured graph replays ONE sample: the
seed and k are kernel arguments).
"""
from __future__ import annotations

import torch

from . import tiled
from .tiled import TiledAdjacency

__all__ = ["FanoutSample", "sample_fanout"]


class FanoutSample:
    """A fixed-fanout sample: the view it was taken on (``view``: ``adj`` samples the rows of A, ``adj.T`` its columns), ``k``, ``seed``
    and ``thr`` (int32 storage of the uint32 thresholds, [n], on the adjacency's device). Cell (i, j) of A is kept when
    ``H(i, j, seed) >= thr[u]`` with u the cell's coordinate on the sampled axis: exactly min(deg, k) cells per node of that axis."""

    def __init__(self, view: TiledAdjacency, k: int, seed: int, thr: torch.Tensor):
        self.view, self.k, self.seed, self.thr = view, k, seed, thr

    def __repr__(self) -> str:
        return f"FanoutSample(k={self.k}, seed={self.seed:#x}, axis={'columns' if self.view.transposed else 'rows'}, n={self.view.n})"


def _check_k_seed(k, seed) -> None:
    if isinstance(k, bool) or not isinstance(k, int):
        raise TypeError(f"fanout's k must be an int >= 1, not {type(k).__name__}")
    if isinstance(seed, bool) or not isinstance(seed, int):
        raise TypeError(f"fanout's seed must be an int in [0, 2^64), not {type(seed).__name__}")
    if k < 1:
        raise ValueError(f"fanout's k must be at least 1, not {k!r}")
    if not 0 <= seed < (1 << 64):
        raise ValueError(f"fanout's seed must lie in [0, 2^64), not {seed!r}")


def check_fanout(adj: TiledAdjacency, fanout) -> None:
    """The refusals of ``fanout=`` itself: a pair (k, seed) with k an int >= 1 and the seed under ``edge_drop``'s rules, or a
    :class:`FanoutSample` of this adjacency (either view). Anything else is a TypeError; a sample of another adjacency a ValueError."""
    if isinstance(fanout, FanoutSample):
        if not isinstance(fanout.view, TiledAdjacency) or tiled._base(fanout.view) is not tiled._base(adj):
            raise ValueError("fanout is a sample of another adjacency")
        _check_k_seed(fanout.k, fanout.seed)
        # the C entries take no length for thr and the kernels index it by node id: this is the only guard of a hand-built sample
        thr = fanout.thr
        if not isinstance(thr, torch.Tensor):
            raise TypeError(f"a FanoutSample's thr must be a torch.Tensor (int32 [{adj.n}]), not {type(thr).__name__}")
        if thr.dtype != torch.int32:
            raise TypeError(f"a FanoutSample's thr must be int32 (the uint32 thresholds' words), not {thr.dtype}")
        if thr.dim() != 1 or thr.numel() != adj.n:
            raise ValueError(f"a FanoutSample's thr must have shape [{adj.n}], not {list(thr.shape)}")
        if thr.device != adj.device:
            raise ValueError(f"a FanoutSample's thr must be on the adjacency's device {adj.device}, not {thr.device}")
        if not thr.is_contiguous():
            raise ValueError("a FanoutSample's thr must be contiguous")
        return
    if not isinstance(fanout, (tuple, list)) or len(fanout) != 2:
        raise TypeError("fanout must be a pair (k, seed), a FanoutSample or None")
    _check_k_seed(*fanout)


def _view_args(adj: TiledAdjacency):
    """(the view's pointers, n_tiles, n) as the C entries take them; an adjacency without tiles passes NULL index pointers."""
    T = adj.n_tiles
    view = (adj.col_ptr, adj.col_tile, adj.col_rb, adj.tiles) if adj.transposed else (adj.row_ptr, adj.kquad, adj.tiles)
    return tuple(t.data_ptr() if T else None for t in view) + (T, adj.n)


def _entry(adj: TiledAdjacency, stem: str):
    return getattr(tiled._c_abi(), stem + ("_t" if adj.transposed else "") + "_fanout")


def _tail(adj: TiledAdjacency, sample: FanoutSample):
    """(thr, thr_of_nbr, seed): own on the view the sample was taken on, nbr on the other. check_fanout has made sure that both views
    belong to one adjacency, so they are told apart by their direction alone."""
    return sample.thr.data_ptr(), int(sample.view.transposed != adj.transposed), sample.seed


def sample_fanout(adj_view: TiledAdjacency, k: int, seed: int) -> FanoutSample:
    """The sample of fanout ``k`` under ``seed`` on the view passed (``adj``: at most k out-neighbours per row of A; ``adj.T``: at most k
    in-neighbours per column): one selection launch on the current stream, no host read. The sample is in the adjacency's own numbering
    (the new ids on a reordered adjacency)."""
    tiled._check(adj_view)
    _check_k_seed(k, seed)
    thr = torch.empty(adj_view.n, dtype=torch.int32, device=adj_view.device)
    L = tiled._c_abi()
    fn = L.qgtc_tiled_fanout_thr_t if adj_view.transposed else L.qgtc_tiled_fanout_thr
    tiled._c_call("the fanout selection", thr, fn, *_view_args(adj_view),
                  min(k, (1 << 31) - 1), seed, thr.data_ptr(), thr.numel())
    return FanoutSample(adj_view, k, seed, thr)


def as_sample(adj: TiledAdjacency, fanout) -> FanoutSample:
    """The checked ``fanout=`` as a sample: a pair is drawn on the view passed (one selection launch), a sample is itself."""
    check_fanout(adj, fanout)
    return fanout if isinstance(fanout, FanoutSample) else sample_fanout(adj, int(fanout[0]), int(fanout[1]))


def _ptr(t):
    return None if t is None else t.data_ptr()


def mm(adj: TiledAdjacency, X: torch.Tensor, row_scale, src_scale, sample: FanoutSample) -> torch.Tensor:
    """qgtc_tiledmm_f32_fanout / _t_fanout: diag(row_scale) . (A sampled) . diag(src_scale) . X, either scale optional; one launch."""
    out = torch.empty_like(X)
    tiled._c_call("the sampled sum", X, _entry(adj, "qgtc_tiledmm_f32"), *_view_args(adj), X.data_ptr(), X.numel(), X.size(1),
                  _ptr(row_scale), _ptr(src_scale), out.data_ptr(), out.numel(), *_tail(adj, sample))
    return out


def extremum(adj: TiledAdjacency, X: torch.Tensor, reduce: str, return_arg: bool, sample: FanoutSample):
    """qgtc_tiledmax_f32_fanout / _t_fanout: (out, arg or None) over the kept neighbours; one launch."""
    out = torch.empty_like(X)
    arg = torch.empty(X.shape, dtype=torch.int32, device=X.device) if return_arg else None
    tiled._c_call("the sampled extremum", X, _entry(adj, "qgtc_tiledmax_f32"), *_view_args(adj), X.data_ptr(), X.numel(), X.size(1),
                  0 if reduce == "max" else 1, out.data_ptr(), out.numel(), _ptr(arg), 0 if arg is None else arg.numel(),
                  *_tail(adj, sample))
    return out, arg


def att_product(adj: TiledAdjacency, X: torch.Tensor, att_own: torch.Tensor, att_nbr: torch.Tensor, slope: float, backward: bool,
                shift: torch.Tensor, inv, sample: FanoutSample):
    """qgtc_tiledatt_f32_fanout / _t_fanout, one launch. Forward: ``shift`` is M [n] and the result (out, m, inv); backward: ``shift`` and
    ``inv`` are the forward's m and inv and the result (out,)."""
    out = torch.empty_like(X)
    m = None if backward else torch.empty(adj.n, dtype=torch.float32, device=adj.device)
    if not backward:
        inv = torch.empty_like(m)
    tiled._c_call("the sampled attention product", X, _entry(adj, "qgtc_tiledatt_f32"), *_view_args(adj), X.data_ptr(), X.numel(),
                  X.size(1), att_own.data_ptr(), att_nbr.data_ptr(), slope, int(backward), shift.data_ptr(), _ptr(m), inv.data_ptr(),
                  out.data_ptr(), out.numel(), *_tail(adj, sample))
    return (out,) if backward else (out, m, inv)


def att_grad(adj: TiledAdjacency, A: torch.Tensor, B: torch.Tensor, att_own: torch.Tensor, att_nbr: torch.Tensor, slope: float,
             nbr_owns: bool, m: torch.Tensor, inv: torch.Tensor, D: torch.Tensor, sample: FanoutSample) -> torch.Tensor:
    """float32 [n] of qgtc_tiledatt_grad_f32_fanout / _t_fanout: the gradient of the out node's score (``nbr_owns`` False, on the
    forward's view) or of the neighbour's (True, on the other view); one launch."""
    out = torch.empty(adj.n, dtype=torch.float32, device=adj.device)
    tiled._c_call("the sampled score gradient", A, _entry(adj, "qgtc_tiledatt_grad_f32"), *_view_args(adj), A.data_ptr(), B.data_ptr(),
                  A.numel(), A.size(1), att_own.data_ptr(), att_nbr.data_ptr(), slope, int(nbr_owns), m.data_ptr(), inv.data_ptr(),
                  D.data_ptr(), out.data_ptr(), out.numel(), *_tail(adj, sample))
    return out


def attention(adj: TiledAdjacency, X: torch.Tensor, att_out: torch.Tensor, att_nbr: torch.Tensor, slope: float, sample: FanoutSample):
    """(out, m, inv): the N = 1 max launch over the KEPT neighbours gives the softmax shift, then one product launch."""
    q = att_nbr.detach().contiguous()
    M = extremum(adj, q.view(adj.n, 1), "max", False, sample)[0].view(adj.n)
    return att_product(adj, X, att_out.detach(), q, slope, False, M, None, sample)


def forward(adj: TiledAdjacency, mode: str, X: torch.Tensor, row_scale, src_scale, reduce: str, return_arg: bool, attn, slope,
            return_stats: bool, fanout):
    """``tiledMMFloat(..., fanout=)`` after its checks, in the modes that are built: "sum", "extremum", "attention" (one head)."""
    sample = as_sample(adj, fanout)
    if mode == "sum":
        return mm(adj, X, row_scale, src_scale, sample)
    if mode == "extremum":
        out, arg = extremum(adj, X, reduce, bool(return_arg), sample)
        return (out, arg) if return_arg else out
    out, m, inv = attention(adj, X, attn[0], attn[1], slope, sample)
    return (out, m, inv) if return_stats else out
