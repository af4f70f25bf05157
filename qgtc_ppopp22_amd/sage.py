"""GraphSAGE on the tiled adjacency (Hamilton et al. 2017): ``lin_self(X) + lin_nbr(agg(X))`` with ``agg`` the mean or the maximum over
the neighbours - all of them, or a fixed-fanout sample of at most ``fanout`` per node drawn fresh every training step inside the tile
walk (``fanout=`` of ``tiled.tiledAggregate``; include/qgtc_fanout.h), or the neighbours a mini-batch block keeps
(``fanout.sample_blocks``; include/qgtc_blocks.h)."""
from __future__ import annotations

import torch

from . import tiled
from .conv import _draw_edge_seed

__all__ = ["SAGEConv"]


class SAGEConv(torch.nn.Module):
    """``forward(A, X, seed=None) = lin_self(X) + lin_nbr(agg(X))`` for a ``TiledAdjacency`` A (either view; the neighbours are the
    view's) and float32 X [n, in_features]; ``lin_self`` carries the bias, ``lin_nbr`` has none.

    X and the result are in the EDGE LIST'S numbering, as with every layer of ``conv``: on an adjacency of
    ``pack_edges_tiled(..., reorder=True)`` the layer reads ``A.to_new(X)``, runs the aggregate and both linear maps there and returns
    ``A.to_old`` of the sum; on any other adjacency the two are the identity and cost nothing. The sample, ``block.rows`` and
    ``block.inputs`` stay in the ADJACENCY'S numbering (``fanout.sample_fanout``): the seed set of a mini-batch goes through
    ``tiled.node_bitmap(A.to_new(flags), A.n)``, and the batch's rows of the result are ``out[flags]``.

    ``aggr="mean"`` is ``tiledAggregate(A, X, row_scale=s)`` with s the reciprocal of the number of terms, correctly rounded (the kernel
    of ``mean_scale``), 0 for a node without neighbours; ``aggr="max"`` is ``tiledAggregate(A, X, reduce="max")`` (+0 without
    neighbours).

    With ``fanout=k`` and in ``train()`` every forward aggregates over a fresh sample of at most k neighbours per node:
    ``fanout=(k, seed)`` with ``seed`` the argument or, when None, 64 bits drawn from torch's CPU generator (as the layers of ``conv``
    draw their ``edge_drop`` seeds); the mean then divides by min(deg, k), the number of kept neighbours. One selection launch per
    forward; the backward reuses the sample. In ``eval()``, and with ``fanout=None``, nothing is sampled and ``seed`` is ignored.

    With ``block=`` (a ``fanout.Block`` of ``fanout.sample_blocks``, on the view passed or the other) the layer runs one hop of a
    mini-batch: the aggregate is taken over ``block.sample`` - the mean divides by the sample's own counts - and nothing is drawn, so the
    layer's ``fanout``, ``seed`` and ``train()`` / ``eval()`` make no difference. Only the rows of ``block.rows`` are part of the batch:
    every other row holds ``lin_self(X[o])`` plus the bias (its aggregate is +0), gets no gradient through the aggregate and is read by
    no later block, because a layer's rows are a subset of the rows before it and the kept neighbours a subset of ``block.inputs``."""

    def __init__(self, in_features: int, out_features: int, aggr: str = "mean", fanout: int | None = None, bias: bool = True):
        super().__init__()
        if aggr not in ("mean", "max"):
            raise ValueError(f'aggr must be "mean" or "max", not {aggr!r}')
        if fanout is not None:
            if isinstance(fanout, bool) or not isinstance(fanout, int):
                raise TypeError(f"fanout must be an int >= 1 or None, not {type(fanout).__name__}")
            if fanout < 1:
                raise ValueError(f"fanout must be at least 1, not {fanout!r}")
        self.aggr, self.fanout = aggr, fanout
        self.lin_self = torch.nn.Linear(in_features, out_features, bias=bias)
        self.lin_nbr = torch.nn.Linear(in_features, out_features, bias=False)

    def sampled_mean_scale(self, A) -> torch.Tensor:
        """float32 [n]: 1 / min(deg, fanout), correctly rounded, 0 where the degree is 0 - the mean over a sample's kept neighbours."""
        return tiled._inv_degree(A.degrees().clamp(max=self.fanout))

    def forward(self, A, X, seed=None, block=None):
        if not isinstance(A, tiled.TiledAdjacency):
            raise NotImplementedError("SAGEConv aggregates on a TiledAdjacency (QGTC.pack_edges_tiled)")
        if block is not None:
            from . import fanout as _fanout

            if not isinstance(block, _fanout.Block):
                raise TypeError(f"block must be a fanout.Block (fanout.sample_blocks), not {type(block).__name__}")
            if not isinstance(block.sample, _fanout.FanoutSample) or block.sample.view is not A:   # counts belong to the sample's view
                raise ValueError("block was sampled on another view than the one passed")
            Xn = A.to_new(X)
            if self.aggr == "max":
                agg = tiled.tiledAggregate(A, Xn, reduce="max", fanout=block.sample)
            else:
                agg = tiled.tiledAggregate(A, Xn, block.sample.mean_scale(), fanout=block.sample)
            return A.to_old(self.lin_self(Xn) + self.lin_nbr(agg))
        kw = {}
        if self.training and self.fanout is not None:
            kw["fanout"] = (self.fanout, _draw_edge_seed() if seed is None else seed)
        Xn = A.to_new(X)
        if self.aggr == "max":
            agg = tiled.tiledAggregate(A, Xn, reduce="max", **kw)
        else:
            agg = tiled.tiledAggregate(A, Xn, self.sampled_mean_scale(A) if kw else A.mean_scale(), **kw)
        return A.to_old(self.lin_self(Xn) + self.lin_nbr(agg))

    def extra_repr(self) -> str:
        return f"aggr={self.aggr}, fanout={self.fanout}"
