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

The sample itself - :class:`FanoutSample`, :func:`sample_fanout` and the checks of ``fanout=`` - is defined in ``tiled.py``, beside the
other values that name the subgraph of a call, with the launchers of the aggregates and their allocations; this module re-exports it
and holds the mini-batch chain on top (:class:`Block`, :func:`frontier`, :func:`sample_blocks`). ``tiled.py`` does not import it. All
launches go to ``torch.cuda.current_stream()`` and read nothing back, so they can be captured into a graph (a captured graph replays ONE
sample: the seed and k are kernel arguments; the masks and thresholds are read on the device, so a replay follows their contents).
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import tiled
from .tiled import FanoutSample, TiledAdjacency, as_sample, check_fanout, sample_fanout, _check_k_seed, _ptr, _view_args   # noqa: F401 (re-exported)

__all__ = ["Block", "FanoutSample", "frontier", "sample_blocks", "sample_fanout"]


class Block(NamedTuple):
    """One layer of a mini-batch (:func:`sample_blocks`): ``rows`` the bitmap of the layer's output nodes, ``sample`` the masked sample
    of their neighbours, ``inputs`` the bitmap of the nodes the layer reads - ``rows`` and every kept neighbour."""
    rows: torch.Tensor
    sample: FanoutSample
    inputs: torch.Tensor


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
    out = torch.empty(view.mask_words, dtype=torch.int32, device=view.device)
    tiled._c_call("the frontier", out, tiled._c_entry("qgtc_tiled_fanout_frontier", False, view), *_view_args(other),
                  sample.thr.data_ptr(), sample.seed, _ptr(sample.row_mask), _ptr(sample.nbr_mask), _ptr(include), view.mask_words,
                  out.data_ptr(), out.numel())
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
