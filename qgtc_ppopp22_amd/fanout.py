"""Fixed-fanout neighbour sampling on the tiled adjacency (include/qgtc_fanout.h): at most ``k`` neighbours per
node, drawn inside the tile walk, so that GraphSAGE-style training needs no second adjacency per step.

:func:`sample_fanout` takes a sample on one view of an adjacency - one selection launch gives ``thr`` uint32 [n], the k-th largest cell
hash of every node of that view (0 where the node has at most k cells) - and returns a :class:`FanoutSample`. ``fanout=`` of
``tiled.tiledMMFloat`` / ``tiled.tiledAggregate`` takes such a sample, or a pair ``(k, seed)`` from which it takes one on the view passed.
On the view it was taken on a sample is used in the OWN form (the thresholds are the output rows'), on the other view in the NBR form (the
thresholds are the neighbours'): the same kept cells either way, which is what a backward needs.

Mini-batch training (include/qgtc_blocks.h): ``sample_fanout(view, k, seed, row_mask=, nbr_mask=)`` samples the
INDUCED subgraph of two node bitmaps (``tiled.node_bitmap``) without re-packing - only the nodes of ``row_mask`` are sampled, among their
neighbours in ``nbr_mask`` - and the sample then carries the masks and ``counts``, the kept neighbours per node; ``fanout=`` of the
aggregates takes such a sample as it takes any other (the masks travel INSIDE the sample, never beside it). :func:`frontier` gives the
nodes a sample's kept edges reach as a bitmap, the next hop's seed set, and :func:`sample_blocks` chains hops into the
:class:`Block` list that ``sage.SAGEConv(block=)`` consumes: two launches a layer.

This module holds the ctypes calls of the entries of both headers and every allocation of the feature; ``tiled.py`` delegates to it. All
launches go to ``torch.cuda.current_stream()`` and read nothing back, so they can be captured into a graph (a captured graph replays ONE
sample: the seed and k are kernel arguments; the masks and thresholds are read on the device, so a replay follows their contents).
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import tiled
from .tiled import TiledAdjacency

__all__ = ["Block", "FanoutSample", "frontier", "sample_blocks", "sample_fanout"]


class FanoutSample:
    """A fixed-fanout sample: the view it was taken on (``view``: ``adj`` samples the rows of A, ``adj.T`` its columns), ``k``, ``seed``
    and ``thr`` (int32 storage of the uint32 thresholds, [n], on the adjacency's device). Cell (i, j) of A is kept when
    ``H(i, j, seed) >= thr[u]`` with u the cell's coordinate on the sampled axis: exactly min(deg, k) cells per node of that axis.

    A MASKED sample (``sample_fanout(..., row_mask=, nbr_mask=)``) also carries the two bitmaps, relative to ``view`` (either may be None:
    all nodes), and ``counts`` int32 [n], the kept neighbours per node: min(deg_m, k) inside ``row_mask``, 0 outside. A cell is then kept
    when its sampled end is in ``row_mask``, its other end in ``nbr_mask`` and the hash test holds."""

    def __init__(self, view: TiledAdjacency, k: int, seed: int, thr: torch.Tensor, row_mask: torch.Tensor | None = None,
                 nbr_mask: torch.Tensor | None = None, counts: torch.Tensor | None = None):
        self.view, self.k, self.seed, self.thr = view, k, seed, thr
        self.row_mask, self.nbr_mask, self.counts = row_mask, nbr_mask, counts

    def mean_scale(self) -> torch.Tensor:
        """float32 [n]: the reciprocal of the number of kept neighbours, correctly rounded, 0 where there are none - ``row_scale`` of the
        mean over the sample on ``view``. Unmasked that is 1 / min(deg, k)."""
        if self.counts is not None:
            return tiled._inv_degree(self.counts)
        if self.row_mask is not None or self.nbr_mask is not None:
            raise ValueError("a masked FanoutSample needs its counts for the mean (sample_fanout returns them)")
        return tiled._inv_degree(self.view.degrees().clamp(max=min(self.k, (1 << 31) - 1)))

    def __repr__(self) -> str:
        masks = "".join(f", {name}" for name, m in (("row_mask", self.row_mask), ("nbr_mask", self.nbr_mask)) if m is not None)
        return (f"FanoutSample(k={self.k}, seed={self.seed:#x}, axis={'columns' if self.view.transposed else 'rows'}, "
                f"n={self.view.n}{masks})")


class Block(NamedTuple):
    """One layer of a mini-batch (:func:`sample_blocks`): ``rows`` the bitmap of the layer's output nodes, ``sample`` the masked sample
    of their neighbours, ``inputs`` the bitmap of the nodes the layer reads - ``rows`` and every kept neighbour."""
    rows: torch.Tensor
    sample: FanoutSample
    inputs: torch.Tensor


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
        for name in ("row_mask", "nbr_mask"):   # bitmaps relative to the sample's view; both views have the adjacency's n and device
            if getattr(fanout, name) is not None:
                tiled._check_mask(adj, getattr(fanout, name), f"a FanoutSample's {name}")
        counts = fanout.counts
        if counts is not None:
            if not isinstance(counts, torch.Tensor):
                raise TypeError(f"a FanoutSample's counts must be a torch.Tensor (int32 [{adj.n}]), not {type(counts).__name__}")
            if counts.dtype != torch.int32:
                raise TypeError(f"a FanoutSample's counts must be int32, not {counts.dtype}")
            if counts.dim() != 1 or counts.numel() != adj.n:
                raise ValueError(f"a FanoutSample's counts must have shape [{adj.n}], not {list(counts.shape)}")
            if counts.device != adj.device:
                raise ValueError(f"a FanoutSample's counts must be on the adjacency's device {adj.device}, not {counts.device}")
            if not counts.is_contiguous():
                raise ValueError("a FanoutSample's counts must be contiguous")
        return
    if not isinstance(fanout, (tuple, list)) or len(fanout) != 2:
        raise TypeError("fanout must be a pair (k, seed), a FanoutSample or None")
    _check_k_seed(*fanout)


def _view_args(adj: TiledAdjacency):
    """(the view's pointers, n_tiles, n) as the C entries take them; an adjacency without tiles passes NULL index pointers."""
    T = adj.n_tiles
    view = (adj.col_ptr, adj.col_tile, adj.col_rb, adj.tiles) if adj.transposed else (adj.row_ptr, adj.kquad, adj.tiles)
    return tuple(t.data_ptr() if T else None for t in view) + (T, adj.n)


def _masked(sample: FanoutSample) -> bool:
    return sample.row_mask is not None or sample.nbr_mask is not None


def _entry(adj: TiledAdjacency, stem: str, sample: FanoutSample):
    """the _fanout entry of the view, or its _fanout_nodes twin (include/qgtc_blocks.h) when the sample carries a mask"""
    return getattr(tiled._c_abi(), stem + ("_t" if adj.transposed else "") + ("_fanout_nodes" if _masked(sample) else "_fanout"))


def _ptr(t):
    return None if t is None else t.data_ptr()


def _mask_words(adj: TiledAdjacency) -> int:
    return (adj.n + 127) // 128 * 4


def _tail(adj: TiledAdjacency, sample: FanoutSample):
    """(thr, thr_of_nbr, seed): own on the view the sample was taken on, nbr on the other. check_fanout has made sure that both views
    belong to one adjacency, so they are told apart by their direction alone. A masked sample adds (row_mask, nbr_mask, mask_words)
    relative to the view walked: its own masks on its own view, the two swapped on the other."""
    nbr = int(sample.view.transposed != adj.transposed)
    tail = (sample.thr.data_ptr(), nbr, sample.seed)
    if _masked(sample):
        masks = (sample.nbr_mask, sample.row_mask) if nbr else (sample.row_mask, sample.nbr_mask)
        tail += (_ptr(masks[0]), _ptr(masks[1]), _mask_words(adj))
    return tail


def sample_fanout(adj_view: TiledAdjacency, k: int, seed: int, row_mask: torch.Tensor | None = None,
                  nbr_mask: torch.Tensor | None = None) -> FanoutSample:
    """The sample of fanout ``k`` under ``seed`` on the view passed (``adj``: at most k out-neighbours per row of A; ``adj.T``: at most k
    in-neighbours per column): one selection launch on the current stream, no host read. The sample is in the adjacency's own numbering
    (the new ids on a reordered adjacency).

    With ``row_mask`` and / or ``nbr_mask`` (bitmaps of ``tiled.node_bitmap``, relative to the view passed) the sample is taken on the
    induced subgraph: only the nodes of ``row_mask`` are sampled, among their neighbours in ``nbr_mask``; a node outside ``row_mask``
    keeps nothing and none of its tiles is read. Still one launch; the sample carries the masks and ``counts``. It is, word for word, the
    unmasked sample of ``pack_edges_tiled`` of the edges between the two sets."""
    tiled._check(adj_view)
    _check_k_seed(k, seed)
    thr = torch.empty(adj_view.n, dtype=torch.int32, device=adj_view.device)
    L = tiled._c_abi()
    if row_mask is None and nbr_mask is None:
        fn = L.qgtc_tiled_fanout_thr_t if adj_view.transposed else L.qgtc_tiled_fanout_thr
        tiled._c_call("the fanout selection", thr, fn, *_view_args(adj_view),
                      min(k, (1 << 31) - 1), seed, thr.data_ptr(), thr.numel())
        return FanoutSample(adj_view, k, seed, thr)
    for name, mask in (("row_mask", row_mask), ("nbr_mask", nbr_mask)):
        if mask is not None:
            tiled._check_mask(adj_view, mask, name)
    counts = torch.empty(adj_view.n, dtype=torch.int32, device=adj_view.device)
    fn = L.qgtc_tiled_fanout_thr_t_nodes if adj_view.transposed else L.qgtc_tiled_fanout_thr_nodes
    tiled._c_call("the masked fanout selection", thr, fn, *_view_args(adj_view), min(k, (1 << 31) - 1), seed, thr.data_ptr(), thr.numel(),
                  counts.data_ptr(), counts.numel(), _ptr(row_mask), _ptr(nbr_mask), _mask_words(adj_view))
    return FanoutSample(adj_view, k, seed, thr, row_mask, nbr_mask, counts)


def frontier(sample: FanoutSample, include=None) -> torch.Tensor:
    """int32 [S128(n) * 4]: the bitmap of the nodes that the kept cells of ``sample`` reach - node v is set iff some node of the sample's
    ``row_mask`` keeps neighbour v - ORed with ``include`` (a bitmap; ``True`` is shorthand for the sample's ``row_mask``, so that a
    layer's inputs contain its outputs). One launch on the current stream, no atomics, no clear, no host read; pad bits are zero. It is
    the next hop's ``row_mask``."""
    if not isinstance(sample, FanoutSample):
        raise TypeError(f"frontier takes a FanoutSample, not {type(sample).__name__}")
    view = sample.view
    tiled._check(view)
    check_fanout(view, sample)
    if include is True:
        include = sample.row_mask
    if include is not None:
        tiled._check_mask(view, include, "include")
    other = view.T   # the output is indexed by the neighbour: the launch walks the other view's index
    out = torch.empty(_mask_words(view), dtype=torch.int32, device=view.device)
    L = tiled._c_abi()
    fn = L.qgtc_tiled_fanout_frontier_t if view.transposed else L.qgtc_tiled_fanout_frontier
    tiled._c_call("the frontier", out, fn, *_view_args(other), sample.thr.data_ptr(), sample.seed, _ptr(sample.row_mask),
                  _ptr(sample.nbr_mask), _ptr(include), _mask_words(view), out.data_ptr(), out.numel())
    return out


_GOLDEN64 = 0x9E3779B97F4A7C15


def sample_blocks(adj_view: TiledAdjacency, seeds: torch.Tensor, fanouts, seed: int) -> list:
    """The blocks of a mini-batch of ``len(fanouts)`` layers on the view passed, input layer FIRST (zip them with the layers):
    ``seeds`` is the bitmap of the batch's output nodes; from the last layer back, ``rows_L = seeds``,
    ``sample_l = sample_fanout(view, fanouts[l], seed_l, row_mask=rows_l)`` and ``rows_{l-1} = frontier(sample_l, include=True)``, with
    ``seed_l = (seed + (L - 1 - l) * 0x9E3779B97F4A7C15) mod 2^64``. Two launches a layer, no host read: the chain can be captured."""
    tiled._check(adj_view)
    tiled._check_mask(adj_view, seeds, "seeds")
    fanouts = list(fanouts)
    if not fanouts:
        raise ValueError("fanouts must name at least one layer")
    for k in fanouts:
        _check_k_seed(k, seed)
    blocks, rows, L = [], seeds, len(fanouts)
    for l in range(L - 1, -1, -1):
        sample = sample_fanout(adj_view, fanouts[l], (seed + (L - 1 - l) * _GOLDEN64) % (1 << 64), row_mask=rows)
        inputs = frontier(sample, include=True)
        blocks.append(Block(rows, sample, inputs))
        rows = inputs
    return blocks[::-1]


def as_sample(adj: TiledAdjacency, fanout) -> FanoutSample:
    """The checked ``fanout=`` as a sample: a pair is drawn on the view passed (one selection launch), a sample is itself."""
    check_fanout(adj, fanout)
    return fanout if isinstance(fanout, FanoutSample) else sample_fanout(adj, int(fanout[0]), int(fanout[1]))


def mm(adj: TiledAdjacency, X: torch.Tensor, row_scale, src_scale, sample: FanoutSample) -> torch.Tensor:
    """qgtc_tiledmm_f32_fanout / _t_fanout: diag(row_scale) . (A sampled) . diag(src_scale) . X, either scale optional; one launch."""
    out = torch.empty_like(X)
    tiled._c_call("the sampled sum", X, _entry(adj, "qgtc_tiledmm_f32", sample), *_view_args(adj), X.data_ptr(), X.numel(), X.size(1),
                  _ptr(row_scale), _ptr(src_scale), out.data_ptr(), out.numel(), *_tail(adj, sample))
    return out


def extremum(adj: TiledAdjacency, X: torch.Tensor, reduce: str, return_arg: bool, sample: FanoutSample):
    """qgtc_tiledmax_f32_fanout / _t_fanout: (out, arg or None) over the kept neighbours; one launch."""
    out = torch.empty_like(X)
    arg = torch.empty(X.shape, dtype=torch.int32, device=X.device) if return_arg else None
    tiled._c_call("the sampled extremum", X, _entry(adj, "qgtc_tiledmax_f32", sample), *_view_args(adj), X.data_ptr(), X.numel(), X.size(1),
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
    tiled._c_call("the sampled attention product", X, _entry(adj, "qgtc_tiledatt_f32", sample), *_view_args(adj), X.data_ptr(), X.numel(),
                  X.size(1), att_own.data_ptr(), att_nbr.data_ptr(), slope, int(backward), shift.data_ptr(), _ptr(m), inv.data_ptr(),
                  out.data_ptr(), out.numel(), *_tail(adj, sample))
    return (out,) if backward else (out, m, inv)


def att_grad(adj: TiledAdjacency, A: torch.Tensor, B: torch.Tensor, att_own: torch.Tensor, att_nbr: torch.Tensor, slope: float,
             nbr_owns: bool, m: torch.Tensor, inv: torch.Tensor, D: torch.Tensor, sample: FanoutSample) -> torch.Tensor:
    """float32 [n] of qgtc_tiledatt_grad_f32_fanout / _t_fanout: the gradient of the out node's score (``nbr_owns`` False, on the
    forward's view) or of the neighbour's (True, on the other view); one launch."""
    out = torch.empty(adj.n, dtype=torch.float32, device=adj.device)
    tiled._c_call("the sampled score gradient", A, _entry(adj, "qgtc_tiledatt_grad_f32", sample), *_view_args(adj), A.data_ptr(), B.data_ptr(),
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
