"""Quantised GCN layers over the QGTC operators — the working counterpart of the reference's
QGTC_conv.py (which is dead code there: it calls `QGTC.bitMM2Bit` with 4 arguments and
`QGTC.val2bit` with 2 against 8- and 4-argument bindings, QGTC_conv.py:15-21,57-64, and
`GCNConv_Qnt.__init__` calls `super(GCNConv, self)`, :40). Same class names and the same two-step
aggregation (QGTC_conv.py:14-22: X·W, then A·(XW)), with the operand layouts the kernels actually
need: X·W is re-packed in the cols layout by `bitMM2Bit_col` so that it can be the right operand of
A·(XW) (what unitest.py:100-109 does).

The quantised layers are inference only, like the reference (its backward is `pass`, QGTC_conv.py:24-27); the float `GCNConv` on a
tile-compressed adjacency is trainable (QGTC.tiledAggregate).
"""
from __future__ import annotations

import torch

import QGTC  # the HIP extension; there is no fallback


def _check_drop_rate(edge_drop) -> float:
    rate = float(edge_drop)
    if not 0.0 <= rate < 1.0:   # a NaN fails both comparisons
        raise ValueError(f"edge_drop must lie in [0, 1), not {edge_drop!r}")
    return rate


def _node_mask(A, nodes) -> torch.Tensor:
    """The bitmap of ``nodes`` (bool [n], in X's numbering) in A's numbering (tiled.node_bitmap)."""
    if not isinstance(nodes, torch.Tensor) or nodes.dtype != torch.bool:
        raise TypeError("nodes must be a bool tensor [n] in X's numbering")
    if nodes.dim() != 1 or nodes.numel() != A.n:
        raise ValueError(f"nodes must have shape [{A.n}], not {list(nodes.shape)}")
    from .tiled import node_bitmap

    return node_bitmap(A.to_new(nodes), A.n)


def _draw_edge_seed() -> int:
    """64 bits from torch's CPU generator (two 32-bit draws): follows torch.manual_seed, touches no device."""
    hi, lo = torch.randint(0, 1 << 32, (2,), dtype=torch.int64).tolist()
    return (hi << 32) | lo


class Aggregation_Qnt(torch.autograd.Function):
    """One quantised GCN layer on packed operands: requant(A · requant(X · W)).

    bit_A : rows layout, 1 bit, [n, n]            bit_X : rows layout, act_bit planes, [n, f_in]
    bit_W : cols layout, w_bit planes, [f_in, f_out]
    `output=False` returns the packed activations (rows layout, act_bit planes, [n, f_out]);
    `output=True` returns float32 [n, f_out] (QGTC_conv.py:19-22)."""

    @staticmethod
    def forward(ctx, bit_A, bit_X, bit_W, n, f_in, f_out, act_bit, w_bit, output=False):
        # one extension call per layer (the library's fused-layer entry, qgtc_gcn_layer_batched): X.W re-packed in the
        # cols layout, then A.(XW); word for word what bitMM2Bit_col followed by bitMM2Bit / bitMM2Int returns
        return QGTC.gcn_layer(bit_A, bit_X, bit_W, n, f_in, f_out, 1, act_bit, w_bit, output)

    @staticmethod
    def backward(ctx, d_output):  # the reference has no training path (QGTC_conv.py:24-27)
        raise NotImplementedError("QGTC layers are inference-only")


class GCNConv_Qnt(torch.nn.Module):
    """Two-layer quantised GCN (QGTC_conv.py:38-78): out = A · q(q(A · q(X·W_in)) · W_out).

    ``aggr="sum"`` is the reference's aggregate. ``aggr="mean"`` divides each aggregate by the row's degree (the rows of the view it
    is given: out-neighbours on ``adj``, in-neighbours on ``adj.T``), in the product kernel's epilogue; it needs a whole graph's
    QGTC.TiledAdjacency, where the plain sum runs into requant's clamp.

    ``float_out=True`` keeps the last layer in full precision: the class scores h . W_out stay the float32 product (bitMM2Int) and
    are aggregated as floats (QGTC.tiledMMFloat) instead of being requantised to ``act_bit`` bits before the neighbours are summed.
    It needs a QGTC.TiledAdjacency too; the first layer is unchanged."""

    def __init__(self, input_dim, hidden_dim, output_dim, num_layers=2, w_bit=2, act_bit=3, aggr="sum", float_out=False):
        super().__init__()
        if aggr not in ("sum", "mean"):
            raise ValueError(f'aggr must be "sum" or "mean", not {aggr!r}')
        self.aggr = aggr
        self.float_out = bool(float_out)
        self.input_dim, self.hidden_dim, self.output_dim = input_dim, hidden_dim, output_dim
        self.W_in = torch.nn.Parameter(torch.randn(input_dim, hidden_dim))
        self.W_out = torch.nn.Parameter(torch.randn(hidden_dim, output_dim))
        self.w_bit = w_bit
        self.act_bit = act_bit
        # edge-list adjacencies: True checks the indices on the device and reads the flag back (one host sync per
        # forward); callers that build their own induced edge lists (sampler.ClusterIter) can switch it off
        self.validate_edges = True
        self.bit_W_in = None    # what the last forward packed (kept for callers that read them); never read back by a forward
        self.bit_W_out = None

    def weight_Qnt(self):
        """Pack the weights (cols layout: they are right operands): two val2bit launches, on [input_dim, hidden_dim] and
        [hidden_dim, output_dim]. forward() calls this EVERY time: torch's version counter misses ``p.data.copy_()``, ``p.data = t``,
        ``vector_to_parameters``, ``half().float()`` and ``load_state_dict(assign=True)``, so nothing short of reading the weights can
        tell that they moved. val2bit runs on the current stream and is capturable: a captured forward follows the weights' contents."""
        self.bit_W_in = QGTC.val2bit(self.W_in.detach().contiguous(), self.w_bit, True, False)
        self.bit_W_out = QGTC.val2bit(self.W_out.detach().contiguous(), self.w_bit, True, False)

    def A_Qnt(self, A):
        """A: dense float [n, n], or a (src, dst, n) edge list (packed without the dense detour)."""
        if isinstance(A, (tuple, list)):
            src, dst, n = A
            return QGTC.pack_edges(src, dst, n, n, 1, self.validate_edges)
        return QGTC.val2bit(A.contiguous(), 1, False, False)

    def X_Qnt(self, X):
        return QGTC.val2bit(X.contiguous(), self.act_bit, False, False)

    def forward(self, A, X, nodes=None):
        """X: node embeddings [n_nodes, n_dim]; A: the subgraph's adjacency (dense or edge list), or a whole graph's
        QGTC.TiledAdjacency (QGTC.pack_edges_tiled).

        ``nodes`` (a bool [n] tensor in X's numbering) runs both layers on the INDUCED subgraph of those nodes, as a Cluster-GCN batch
        does, on the whole graph's QGTC.TiledAdjacency and without packing anything: both aggregates take
        ``row_mask = nbr_mask = tiled.node_bitmap(A.to_new(nodes), n)`` (``tiledMM2Bit`` / ``tiledMM2Int``; ``tiledMMFloat`` under
        ``float_out``) and ``aggr="mean"`` takes the induced degrees (``A.mean_scale(row_mask=, nbr_mask=)``). For the rows in ``nodes``
        the result is bit for bit the same layer on ``pack_edges_tiled`` of the edges between the nodes; a row outside holds what that
        layer gives an isolated node. With a dense or edge-list ``A`` it is a NotImplementedError. A masked aggregate of a contiguous
        or community-aligned eighth of the nodes measured 0.05 - 0.39 of the whole-graph launch; a random node set leaves every block
        live and can cost more than the whole-graph launch."""
        if self.aggr not in ("sum", "mean"):   # read at every forward: the constructor's refusal holds for a reassigned value too
            raise ValueError(f'aggr must be "sum" or "mean", not {self.aggr!r}')
        self.weight_Qnt()
        assert X.device == self.W_in.device, "inputs and weights must be on the same device"
        n = X.size(0)
        if isinstance(A, QGTC.TiledAdjacency):
            return self._forward_tiled(A, X, nodes)
        if nodes is not None:
            raise NotImplementedError("nodes needs a QGTC.TiledAdjacency (QGTC.pack_edges_tiled), not a dense A")
        if self.aggr == "mean":
            raise NotImplementedError('aggr="mean" needs a QGTC.TiledAdjacency (QGTC.pack_edges_tiled), not a dense or edge-list A')
        if self.float_out:
            raise NotImplementedError("float_out=True needs a QGTC.TiledAdjacency (QGTC.pack_edges_tiled), not a dense or edge-list A")
        bit_A = self.A_Qnt(A)
        bit_X = self.X_Qnt(X)
        bit_h = Aggregation_Qnt.apply(bit_A, bit_X, self.bit_W_in, n, self.input_dim, self.hidden_dim,
                                      self.act_bit, self.w_bit, False)
        return Aggregation_Qnt.apply(bit_A, bit_h, self.bit_W_out, n, self.hidden_dim, self.output_dim,
                                     self.act_bit, self.w_bit, True)

    def _forward_tiled(self, A, X, nodes=None):
        """The same two layers with the tile-compressed aggregate: per layer X.W re-packed in the cols layout
        (bitMM2Bit_col), then tiledMM2Bit / tiledMM2Int - the words gcn_layer gives on the dense adjacency. A reordered
        adjacency (A.perm set) gets X in its numbering and gives the output back in X's: every term moves with its node and the
        quantisers work element by element, so the result is bit-identical to the unreordered one. With aggr="mean" both aggregates
        take A.mean_scale() as their row scale (it lives in A's numbering and follows the view). With float_out the last layer is
        tiledMMFloat on the float32 product h . W_out (bitMM2Int). Its adds follow A's numbering; the class scores are integers, so
        as long as the sums stay below 2^24 every add is exact and a reordered adjacency still gives the unreordered bits. With
        ``nodes`` the bitmap of the node set is the row and the neighbour mask of both aggregates and of the mean's degrees; without
        it the calls are the ones they always were."""
        n = X.size(0)
        assert A.n == n, "the adjacency and X must have the same number of nodes"
        bm = None if nodes is None else _node_mask(A, nodes)
        X = A.to_new(X)
        bit_X = self.X_Qnt(X)
        t = QGTC.bitMM2Bit_col(bit_X, self.bit_W_in, n, self.input_dim, self.hidden_dim, self.act_bit, self.w_bit, self.act_bit)
        if bm is None:
            scale = A.mean_scale() if self.aggr == "mean" else None
            bit_h = QGTC.tiledMM2Bit(A, t, self.hidden_dim, self.act_bit, self.act_bit, scale)
        else:
            scale = A.mean_scale(row_mask=bm, nbr_mask=bm) if self.aggr == "mean" else None
            bit_h = QGTC.tiledMM2Bit(A, t, self.hidden_dim, self.act_bit, self.act_bit, scale, row_mask=bm, nbr_mask=bm)
        if self.float_out:
            hw = QGTC.bitMM2Int(bit_h, self.bit_W_out, n, self.hidden_dim, self.output_dim, self.act_bit, self.w_bit)
            if bm is None:
                return A.to_old(QGTC.tiledMMFloat(A, hw, scale))
            return A.to_old(QGTC.tiledMMFloat(A, hw, scale, row_mask=bm, nbr_mask=bm))
        t = QGTC.bitMM2Bit_col(bit_h, self.bit_W_out, n, self.hidden_dim, self.output_dim, self.act_bit, self.w_bit, self.act_bit)
        if bm is None:
            return A.to_old(QGTC.tiledMM2Int(A, t, self.output_dim, self.act_bit, scale))
        return A.to_old(QGTC.tiledMM2Int(A, t, self.output_dim, self.act_bit, scale, row_mask=bm, nbr_mask=bm))


class GCNConv(torch.nn.Module):
    """The float reference layer pair of QGTC_conv.py:101-121 (A · ((A · (X·W_in)) · W_out)).

    Given a whole graph's QGTC.TiledAdjacency the two aggregates are QGTC.tiledAggregate (float32, differentiable: the layer pair is
    trainable), under ``norm``: None the plain sum, "mean" D^-1 . A (``A.mean_scale()`` on the output row), "sym" the GCN
    normalisation D_out^-1/2 . A . D_in^-1/2 (``A.sym_scale()`` on the output row, ``A.T.sym_scale()`` on the neighbour being added;
    on a symmetric edge list, D^-1/2 . A . D^-1/2 - QGTC.add_self_loops gives the A + I of Kipf and Welling). A dense ``A`` takes
    ``norm=None`` only.

    ``aggr`` is the reducer of both aggregates: "sum" (the default, under ``norm``), or "max" / "min", the element-wise extremum over
    the neighbours (``tiledAggregate(reduce=)``; the gradient goes to the neighbour that won). An extremum has no normalisation, so
    "max" / "min" with a ``norm`` is a ValueError, and it needs a QGTC.TiledAdjacency. ``norm``, ``aggr`` and ``edge_drop`` are read at
    every forward and may be reassigned on a live layer; the same refusals hold then (``edge_drop`` where it is assigned, the other two
    at the next forward).

    ``edge_drop`` (a rate in [0, 1), default 0) is DropEdge on a QGTC.TiledAdjacency: in training mode both aggregates of a forward run
    on one random subgraph, ``tiledAggregate(..., edge_drop=(edge_drop, seed))`` with one seed per forward - ``edge_seed`` of
    :meth:`forward` when given, otherwise 64 bits drawn from torch's CPU generator (no device synchronisation; ``torch.manual_seed``
    makes it repeatable). With ``aggr="sum"`` only, the row scale of both aggregates is multiplied by ``keep_scale``, the float32 nearest
    1 / (1 - edge_drop) (for ``norm=None`` the row scale is that constant vector), which keeps the aggregate unbiased with the FULL
    graph's degrees in ``norm``; "max" / "min" rescale nothing and never read ``keep_scale``. ``edge_seed`` is checked where it is used, by ``tiledAggregate``. The mask lives in A's own numbering (``tiledMMFloat``). In eval mode
    the layer is the one without ``edge_drop``, bit for bit.

    ``nodes`` of :meth:`forward` (a bool [n] tensor in X's numbering) runs the layer pair on the INDUCED subgraph of those nodes, as a
    Cluster-GCN batch does, on the whole graph's QGTC.TiledAdjacency and without packing anything: both aggregates take
    ``row_mask = nbr_mask = tiled.node_bitmap(A.to_new(nodes), n)`` and ``norm`` takes the induced degrees (``A.mean_scale(row_mask=,
    nbr_mask=)`` / ``sym_scale``). Rows outside ``nodes`` come back +0; the result is bit for bit the same layer on
    ``pack_edges_tiled`` of the edges between the nodes. With an active ``edge_drop`` (training mode, rate > 0) or a dense ``A`` it is
    a NotImplementedError.

    ``edge_weight`` of :meth:`forward` (float32 [nnz] in slot order, ``tiled.edge_values``) weighs every edge of a
    QGTC.TiledAdjacency: both aggregates are ``tiledAggregate(..., edge_weight=)``, differentiable in the weights too. It is accepted
    with ``norm=None`` and ``aggr="sum"`` only and without ``nodes`` or an active ``edge_drop``; anything else is a ValueError: normalise
    the weights beforehand (``tiled.edge_endpoints`` gives every slot's row and column)."""

    def __init__(self, input_dim, hidden_dim, output_dim, num_layers=2, norm=None, aggr="sum", edge_drop=0.0):
        super().__init__()
        self.edge_drop = edge_drop
        self._keep_vector = None   # norm=None under the mask: (keep_scale, the vector holding it on every row), per (n, device, keep_scale)
        self.norm = norm
        self.aggr = aggr
        self._check_config()
        self.W_in = torch.nn.Parameter(torch.randn(input_dim, hidden_dim))
        self.W_out = torch.nn.Parameter(torch.randn(hidden_dim, output_dim))

    @property
    def edge_drop(self) -> float:
        return self._edge_drop

    @edge_drop.setter
    def edge_drop(self, rate):
        """``layer.edge_drop = r`` anneals DropEdge: the rate is checked here, and ``keep_scale`` is computed from it."""
        self._edge_drop = _check_drop_rate(rate)

    @property
    def keep_scale(self) -> float:
        """The float32 nearest 1 / (1 - edge_drop), as a Python float: always of the rate the layer holds now."""
        return float(torch.tensor(1.0 / (1.0 - self._edge_drop), dtype=torch.float64).to(torch.float32))

    def _check_config(self):
        """``norm`` and ``aggr`` are read at every forward and may be reassigned: the constructor's refusals hold there too."""
        if self.norm not in (None, "mean", "sym"):
            raise ValueError(f'norm must be None, "mean" or "sym", not {self.norm!r}')
        if self.aggr not in ("sum", "max", "min"):
            raise ValueError(f'aggr must be "sum", "max" or "min", not {self.aggr!r}')
        if self.aggr != "sum" and self.norm is not None:
            raise ValueError(f'aggr="{self.aggr}" takes no norm (norm={self.norm!r}): an extremum is not scaled')

    def forward(self, A, X, edge_seed=None, nodes=None, edge_weight=None):
        self._check_config()
        if isinstance(A, QGTC.TiledAdjacency):
            if edge_weight is not None:
                return self._forward_weighted(A, X, edge_weight, nodes)
            return self._forward_tiled(A, X, edge_seed, nodes)
        if edge_weight is not None:
            raise ValueError("edge_weight needs a QGTC.TiledAdjacency (QGTC.pack_edges_tiled), not a dense A: put the weights into A")
        if nodes is not None:
            raise NotImplementedError("nodes needs a QGTC.TiledAdjacency (QGTC.pack_edges_tiled), not a dense A")
        if self.training and self.edge_drop > 0.0:
            raise NotImplementedError("edge_drop needs a QGTC.TiledAdjacency (QGTC.pack_edges_tiled), not a dense A")
        if self.norm is not None:
            raise NotImplementedError(f'norm="{self.norm}" needs a QGTC.TiledAdjacency (QGTC.pack_edges_tiled), not a dense A')
        if self.aggr != "sum":
            raise NotImplementedError(f'aggr="{self.aggr}" needs a QGTC.TiledAdjacency (QGTC.pack_edges_tiled), not a dense A')
        return torch.mm(A, torch.mm(torch.mm(A, torch.mm(X, self.W_in)), self.W_out))

    def _keep_row_scale(self, A, row):
        """``row`` times keep_scale (one float32 multiply an element); for norm=None the constant vector, cached."""
        keep = self.keep_scale
        if row is not None:
            return row * keep
        cached = self._keep_vector
        if cached is None or cached[0] != keep or cached[1].numel() != A.n or cached[1].device != A.device:
            cached = self._keep_vector = (keep, torch.full((A.n,), keep, dtype=torch.float32, device=A.device))
        return cached[1]

    def _forward_weighted(self, A, X, edge_weight, nodes=None):
        """agg(agg(X . W_in) . W_out) with agg = tiledAggregate(edge_weight=): the plain weighted sum, nothing else."""
        assert A.n == X.size(0), "the adjacency and X must have the same number of nodes"
        for what, on in ((f"norm={self.norm!r}", self.norm is not None), (f'aggr="{self.aggr}"', self.aggr != "sum"),
                         ("nodes", nodes is not None), ("an active edge_drop", self.training and self.edge_drop > 0.0)):
            if on:
                raise ValueError(f"edge_weight cannot be combined with {what}: not built - normalise the weights beforehand "
                                 "(tiled.edge_endpoints gives every slot's row and column)")
        h = QGTC.tiledAggregate(A, torch.mm(A.to_new(X), self.W_in), edge_weight=edge_weight)
        return A.to_old(QGTC.tiledAggregate(A, torch.mm(h, self.W_out), edge_weight=edge_weight))

    def _forward_tiled(self, A, X, edge_seed=None, nodes=None):
        """agg(agg(X . W_in) . W_out) with agg = tiledAggregate under ``norm`` / ``aggr``; X moves to A's numbering and the result
        back. In training with edge_drop > 0 both aggregates take the same (edge_drop, seed). With ``nodes`` both aggregates run on
        the induced subgraph (one bitmap as row and neighbour mask) and ``norm`` takes its degrees."""
        assert A.n == X.size(0), "the adjacency and X must have the same number of nodes"
        drop = None
        if self.training and self.edge_drop > 0.0:
            drop = (self.edge_drop, _draw_edge_seed() if edge_seed is None else edge_seed)
        mask = {}
        if nodes is not None:
            if drop is not None:
                raise NotImplementedError("nodes cannot be combined with an active edge_drop: not built")
            bm = _node_mask(A, nodes)
            mask = {"row_mask": bm, "nbr_mask": bm}
        if self.aggr != "sum":
            h = QGTC.tiledAggregate(A, torch.mm(A.to_new(X), self.W_in), reduce=self.aggr, edge_drop=drop, **mask)
            return A.to_old(QGTC.tiledAggregate(A, torch.mm(h, self.W_out), reduce=self.aggr, edge_drop=drop, **mask))
        row = src = None
        if self.norm == "mean":
            row = A.mean_scale(**mask)
        elif self.norm == "sym":
            row, src = A.sym_scale(**mask), A.T.sym_scale(**mask)
        if drop is not None:
            row = self._keep_row_scale(A, row)
        h = QGTC.tiledAggregate(A, torch.mm(A.to_new(X), self.W_in), row, src, edge_drop=drop, **mask)
        return A.to_old(QGTC.tiledAggregate(A, torch.mm(h, self.W_out), row, src, edge_drop=drop, **mask))


class GATConv(torch.nn.Module):
    """One graph attention layer (Velickovic et al., 2018) on a whole graph's QGTC.TiledAdjacency: h = X . W, and per head the
    softmax-weighted sum of the neighbours' h with the edge logits leaky_relu(a_dst . h_i + a_src . h_j)
    (``QGTC.tiledAggregate(A, h_head, attn=(p, q))`` with p = h_head . a_dst, q = h_head . a_src: no per-edge tensor exists). The
    heads are concatenated ([n, heads * output_dim]) or, with ``concat=False``, averaged ([n, output_dim]). Trainable in W, a_dst and
    a_src. ``A`` is the view whose rows are the receiving nodes: ``adj`` aggregates over out-neighbours, ``adj.T`` over in-neighbours;
    on a reordered adjacency X moves to its numbering and the result back. Self loops are the edge list's business
    (QGTC.add_self_loops). All heads share one ``tiledAggregate`` call with scores [n, heads] (include/qgtc_attn_heads.h): two launches
    forward and five backward for the whole layer, each head bit for bit what the single-head call gives on its slice.

    ``edge_drop`` (a rate in [0, 1), default 0) is neighbourhood dropout: in training mode every head's softmax runs over one random
    subgraph, ``tiledAggregate(..., attn=, edge_drop=(edge_drop, seed))`` with one seed per forward for all heads - ``edge_seed`` of
    :meth:`forward` when given, otherwise 64 bits drawn from torch's CPU generator (no device synchronisation). The softmax
    renormalises over the kept neighbours by itself, so nothing is rescaled; a node that loses every neighbour gives +0. The mask
    lives in A's own numbering (``tiledMMFloat``). In eval mode the layer is the one without ``edge_drop``, bit for bit.

    ``nodes`` of :meth:`forward` (a bool [n] tensor in X's numbering) runs every head on the induced subgraph of those nodes
    (``row_mask = nbr_mask``, as in :class:`GCNConv`): rows outside come back +0, and the result is bit for bit the layer on
    ``pack_edges_tiled`` of the edges between the nodes. With an active ``edge_drop`` it is a NotImplementedError."""

    def __init__(self, input_dim, output_dim, heads=1, negative_slope=0.2, concat=True, edge_drop=0.0):
        super().__init__()
        self.edge_drop = _check_drop_rate(edge_drop)
        if int(heads) < 1:
            raise ValueError(f"heads must be at least 1, not {heads!r}")
        if not 0.0 <= float(negative_slope) <= 1.0:
            raise ValueError(f"negative_slope must lie in [0, 1], not {negative_slope!r}")
        self.input_dim, self.output_dim, self.heads = int(input_dim), int(output_dim), int(heads)
        self.negative_slope, self.concat = float(negative_slope), bool(concat)
        self.W = torch.nn.Parameter(torch.randn(self.input_dim, self.heads * self.output_dim) / self.input_dim ** 0.5)
        self.a_dst = torch.nn.Parameter(torch.randn(self.heads, self.output_dim) / self.output_dim ** 0.5)
        self.a_src = torch.nn.Parameter(torch.randn(self.heads, self.output_dim) / self.output_dim ** 0.5)

    def forward(self, A, X, edge_seed=None, nodes=None):
        if not isinstance(A, QGTC.TiledAdjacency):
            raise NotImplementedError("GATConv needs a QGTC.TiledAdjacency (QGTC.pack_edges_tiled), not a dense or edge-list A")
        assert A.n == X.size(0), "the adjacency and X must have the same number of nodes"
        h = torch.mm(A.to_new(X), self.W)
        drop = None
        if self.training and self.edge_drop > 0.0:
            drop = (self.edge_drop, _draw_edge_seed() if edge_seed is None else edge_seed)
        mask = {}
        if nodes is not None:
            if drop is not None:
                raise NotImplementedError("nodes cannot be combined with an active edge_drop: not built")
            bm = _node_mask(A, nodes)
            mask = {"row_mask": bm, "nbr_mask": bm}
        his, ps, qs = [], [], []
        for i in range(self.heads):
            hi = h[:, i * self.output_dim:(i + 1) * self.output_dim].contiguous()
            his.append(hi)
            ps.append(torch.mv(hi, self.a_dst[i]))
            qs.append(torch.mv(hi, self.a_src[i]))
        if self.heads == 1:
            return A.to_old(QGTC.tiledAggregate(A, his[0], attn=(ps[0], qs[0]), negative_slope=self.negative_slope, edge_drop=drop, **mask))
        # One call for all heads. The scores are stacked before the heads' slices are joined, and both after every torch.mv: autograd
        # then hands a slice its three gradients in the order the loop over heads did - the aggregate's, a_src's, a_dst's - so the
        # sums keep their association and the layer its bits.
        P, Q = torch.stack(ps, dim=1), torch.stack(qs, dim=1)
        out = QGTC.tiledAggregate(A, torch.cat(his, dim=1), attn=(P, Q), negative_slope=self.negative_slope, edge_drop=drop, **mask)
        if not self.concat:   # the mean over the heads, in the layout and order of torch.stack(heads).mean(dim=0)
            out = out.view(A.n, self.heads, self.output_dim).transpose(0, 1).contiguous().mean(dim=0)
        return A.to_old(out)


class TransformerConv(torch.nn.Module):
    """One dot-product attention layer on a whole graph's QGTC.TiledAdjacency (the message passing of a graph Transformer, Shi et al.,
    2021, without its skip connection): q = X . W_q, k = X . W_k, v = X . W_v, and per head the receiving node i takes
    ``sum over its neighbours j of softmax_j(q_i . k_j / sqrt(output_dim)) * v_j`` - ``tiled.tiledEdgeAttention(A, q_head, k_head,
    v_head)``: an SDDMM, the edge softmax and the weighted sum, every launch of forward and backward specified to the bit and without
    atomics. All heads share one call, ``tiledEdgeAttention(A, q, k, v, heads=heads)``: three launches forward and five backward for the
    whole layer, reading q, k and v in place (head h is their columns h * output_dim ..), each head bit for bit what the single-head
    call gives on its slice. The heads are concatenated ([n, heads * output_dim]) or, with ``concat=False``, averaged
    ([n, output_dim]). Trainable in W_q, W_k and W_v. ``A`` is the view whose rows are the receiving nodes: ``adj`` attends over
    out-neighbours, ``adj.T`` over in-neighbours; on a reordered adjacency X moves to its numbering and the result back. A node without
    neighbours gives +0; self loops are the edge list's business (QGTC.add_self_loops).

    There is no dropout and there are no node masks: the aggregate takes the weights through ``edge_weight``, which accepts neither."""

    def __init__(self, input_dim, output_dim, heads=1, concat=True):
        super().__init__()
        if int(heads) < 1:
            raise ValueError(f"heads must be at least 1, not {heads!r}")
        self.input_dim, self.output_dim, self.heads, self.concat = int(input_dim), int(output_dim), int(heads), bool(concat)
        for name in ("W_q", "W_k", "W_v"):
            setattr(self, name, torch.nn.Parameter(torch.randn(self.input_dim, self.heads * self.output_dim) / self.input_dim ** 0.5))

    def forward(self, A, X):
        if not isinstance(A, QGTC.TiledAdjacency):
            raise NotImplementedError("TransformerConv needs a QGTC.TiledAdjacency (QGTC.pack_edges_tiled), not a dense or edge-list A")
        assert A.n == X.size(0), "the adjacency and X must have the same number of nodes"
        from .tiled import tiledEdgeAttention

        Xn = A.to_new(X)
        q, k, v = torch.mm(Xn, self.W_q), torch.mm(Xn, self.W_k), torch.mm(Xn, self.W_v)
        out = tiledEdgeAttention(A, q, k, v, heads=self.heads)
        if self.heads > 1 and not self.concat:   # the mean over the heads, in the layout and order of torch.stack(heads).mean(dim=0)
            out = out.view(A.n, self.heads, self.output_dim).transpose(0, 1).contiguous().mean(dim=0)
        return A.to_old(out)


class GATv2Conv(torch.nn.Module):
    """One GATv2 layer (Brody et al., 2022) on a whole graph's QGTC.TiledAdjacency: hl = X . W_l, hr = X . W_r, and per head the
    receiving node o takes ``sum over its neighbours k of softmax_k(att . leaky_relu(hr_o + hl_k)) * hl_k`` -
    ``tiled.tiledEdgeAdditiveAttention(A, hr, hl, hl, att, negative_slope, heads)``: the additive score (include/qgtc_addscore.h), the
    edge softmax and the weighted sum, three launches forward and five backward for all heads, every one specified to the bit and
    without atomics. Unlike GATConv's ``attn=(p, q)`` logit, the nonlinearity sits before the reduction with ``att``, so the ranking of
    the neighbours depends on the receiving node ("dynamic" attention). With ``share_weights`` W_r is W_l: the matrix is registered once,
    as ``W_l`` (``state_dict()`` has no "W_r"), and ``layer.W_r`` reads it. The heads are concatenated
    ([n, heads * output_dim]) or, with ``concat=False``, averaged ([n, output_dim]), exactly as TransformerConv does. Trainable in W_l,
    W_r and att ([heads, output_dim]). ``A`` is the view whose rows are the receiving nodes: ``adj`` attends over out-neighbours,
    ``adj.T`` over in-neighbours; on a reordered adjacency X moves to its numbering and the result back. A node without neighbours
    gives +0; self loops are the edge list's business (QGTC.add_self_loops).

    There is no ``edge_drop`` and there are no ``nodes``: the aggregate takes the weights through ``edge_weight``, which accepts
    neither."""

    def __init__(self, input_dim, output_dim, heads=1, negative_slope=0.2, concat=True, share_weights=False):
        super().__init__()
        if int(heads) < 1:
            raise ValueError(f"heads must be at least 1, not {heads!r}")
        slope = float(negative_slope)
        if not 0.0 <= slope <= 1.0:
            raise ValueError(f"negative_slope must lie in [0, 1], not {negative_slope!r}")
        self.input_dim, self.output_dim, self.heads, self.concat = int(input_dim), int(output_dim), int(heads), bool(concat)
        self.negative_slope, self.share_weights = slope, bool(share_weights)
        self.W_l = torch.nn.Parameter(torch.randn(self.input_dim, self.heads * self.output_dim) / self.input_dim ** 0.5)
        if not self.share_weights:   # shared: ONE registered name, so a state dict has one tensor for it (see __getattr__)
            self.W_r = torch.nn.Parameter(torch.randn(self.input_dim, self.heads * self.output_dim) / self.input_dim ** 0.5)
        self.att = torch.nn.Parameter(torch.randn(self.heads, self.output_dim) / self.output_dim ** 0.5)

    def __getattr__(self, name):
        # With share_weights W_r is whatever W_l is now - also after load_state_dict(assign=True) replaced it. A second registered
        # name for the one Parameter would give state_dict() two keys, and loading two differing tensors would keep the last silently.
        if name == "W_r" and self.__dict__.get("share_weights"):
            return self.W_l
        return super().__getattr__(name)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        """A shared layer takes a "W_r" entry only when it equals "W_l" (checkpoints of shared layers from before carried both keys);
        two differing tensors for the one matrix are an error, never a silent choice."""
        if self.share_weights and prefix + "W_r" in state_dict:
            left, right = state_dict.get(prefix + "W_l"), state_dict[prefix + "W_r"]
            if left is not None and left.shape == right.shape and torch.equal(left.to(right.device), right):
                state_dict.pop(prefix + "W_r")   # load_state_dict works on its own shallow copy of the caller's dict
            else:
                error_msgs.append(f'"{prefix}W_r" differs from "{prefix}W_l", and this layer has share_weights=True: it holds one matrix')
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    def forward(self, A, X):
        if not isinstance(A, QGTC.TiledAdjacency):
            raise NotImplementedError("GATv2Conv needs a QGTC.TiledAdjacency (QGTC.pack_edges_tiled), not a dense or edge-list A")
        assert A.n == X.size(0), "the adjacency and X must have the same number of nodes"
        from .tiled import tiledEdgeAdditiveAttention

        Xn = A.to_new(X)
        hl = torch.mm(Xn, self.W_l)
        hr = hl if self.share_weights else torch.mm(Xn, self.W_r)
        out = tiledEdgeAdditiveAttention(A, hr, hl, hl, self.att, self.negative_slope, heads=self.heads)
        if self.heads > 1 and not self.concat:   # the mean over the heads, in the layout and order of torch.stack(heads).mean(dim=0)
            out = out.view(A.n, self.heads, self.output_dim).transpose(0, 1).contiguous().mean(dim=0)
        return A.to_old(out)
