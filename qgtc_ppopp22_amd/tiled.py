"""Tile-compressed 1-bit adjacency of a whole graph (include/qgtc.h, "Tile-compressed adjacency"; DESIGN.md sections 4, 6.10).

The dense route packs an n x n adjacency into n^2/8 bytes and stops at n = 185 363 (4 GiB per packed operand). A
:class:`TiledAdjacency` keeps only the occupied 32-row x 128-column tiles, block-sparse like BSR, and
:func:`tiledMM2Bit` / :func:`tiledMM2Int` multiply from that storage: word for word what ``bitMM2Bit`` / ``bitMM2Int`` give
on ``pack_edges(src, dst, n, n, 1)`` of the same edge list. ``QGTC`` re-exports the functions and the class.

The format is compact only when a node's neighbours have nearby ids. :func:`reorder_nodes` renumbers the nodes of an edge list with
any ids on the device (include/qgtc.h, "Node reordering"), and ``pack_edges_tiled(..., reorder=True)`` packs the graph in that
numbering; the adjacency then carries ``perm`` / ``rank`` and moves tensors between the two numberings.

The rows are sources, so ``tiledMM2Int(adj, X)[s]`` sums X over the out-neighbours of s. ``adj.T`` is the transposed adjacency
(include/qgtc.h, "Transposed tiled adjacency"): the same tiles, listed by k-quad through a small column index built on the device on
first use, and the same functions on it give A^T . X, the in-neighbour sum of message passing (``copy_u`` + ``sum``), word for word
what they give on ``pack_edges_tiled(dst, src, n)``.

Both take ``row_scale`` (include/qgtc.h, "Scaled tiled products and degrees"): a float32 [n] the kernel multiplies every output row by
before the output is formed. With ``adj.mean_scale()``, the reciprocal of ``adj.degrees()``, that is the MEAN over neighbours, which
stays in 0 .. 2^bit2 - 1 where the plain sum of a whole graph runs into requant's clamp.

:func:`tiledMMFloat` aggregates a float32 matrix over the same tiles, on ``adj`` and ``adj.T`` (include/qgtc.h, "Float tiled
products"): each output row adds its neighbours' rows in ascending id order, one float32 add each, so the result is a function of the
inputs alone. With ``src_scale`` every neighbour's row is multiplied by its own factor as it is added (include/qgtc.h, "Source scale"):
``row_scale=adj.sym_scale(), src_scale=adj.T.sym_scale()`` is the GCN normalisation D^-1/2 . A . D^-1/2 in one launch.
:func:`tiledAggregate` is the same product under ``torch.autograd``: its backward is the product on the other view with the two scales
swapped, one launch too. :func:`add_self_loops` prepares an edge list for it.

``reduce="max"`` / ``"min"`` on both functions replace the sum by the element-wise extremum over the neighbours (include/qgtc.h,
"Extremum tiled products"): the value is a neighbour's own word, the lowest id wins a tie and the first NaN wins outright, a row
without neighbours gives +0. ``return_arg=True`` also returns the winning neighbour of every element (int32, -1 for none), and
:func:`tiledAggregate` routes the gradient to exactly that neighbour with one gather on the other view - no atomics, the same bits on
every launch.

``attn=(att_out, att_nbr)`` on both functions is the reducer of GAT (include/qgtc.h, "Attention tiled products"): every row is the
softmax-weighted sum of its neighbours' rows, the weight of edge (o, k) being the softmax over o's neighbours of
``leaky_relu(att_out[o] + att_nbr[k])``. No per-edge value is stored: the weight is rebuilt from the two per-node scores inside the tile
walk, with an exponential that is a fixed sequence of float32 operations, so forward and all three gradients (X and both scores, each a
fold in ascending id order on ``adj`` or ``adj.T``, no atomics) are specified to the bit. ``conv.GATConv`` is the layer on top. With
scores of shape [n, H] (head-minor; include/qgtc_attn_heads.h) the same launches carry H HEADS: head h is the columns h d .. (h + 1) d - 1
of X and of the result, the statistics are [n, H], and every head is bit for bit what the single-head call gives on its contiguous
slice - two launches forward and five backward for all heads, under ``edge_drop`` and node masks as for one head.

``edge_drop=(rate, seed)`` on both functions, in every mode, aggregates over a random subgraph instead (include/qgtc.h, "Edge dropout"):
cell (i, j) of the adjacency survives when a fixed 32-bit hash of (i, j, seed) is at least ``floor(rate * 2^32)``, decided inside the tile
walk on either view, so nothing per edge is stored, no second adjacency is packed and the backward on the other view sees exactly the
forward's subgraph. The result is bit for bit that of the same call on an adjacency packed from the kept edges.

``row_mask`` / ``nbr_mask`` on both functions, in every mode, aggregate over an induced subgraph without packing a second
adjacency (include/qgtc.h, "Node masks"): each is a bitmap from :func:`node_bitmap` or None = all nodes, relative to the view like the
scales. A row outside ``row_mask`` comes back +0, a neighbour outside ``nbr_mask`` is never loaded, a block of 32 rows (128 on ``adj.T``)
without a live row reads no tile, and the result is bit for bit the unmasked call on ``pack_edges_tiled`` of the edges between the two
sets. The backward takes the two masks swapped. ``adj.degrees()``, ``mean_scale()`` and ``sym_scale()`` take the same two keywords and
give the masked graph's. That covers Cluster-GCN batches on the whole-graph adjacency (``conv.GCNConv.forward(nodes=)``), a last layer
on the labelled nodes only, and node dropout. Every mode takes them: under "max" / "min" a row outside ``row_mask`` has arg -1, and the
attention's softmax runs over the participating neighbours. :func:`tiledMM2Bit` / :func:`tiledMM2Int` take the same two keywords
(include/qgtc_bitnodes.h; the launch and its output allocation live in ``tiled_bit.py``): the quantised products on the induced subgraph,
word for word those on the re-packed adjacency, and ``conv.GCNConv_Qnt.forward(nodes=)`` on top.

``edge_weight=values`` on :func:`tiledMMFloat` / :func:`tiledAggregate` (sum only) weighs every edge (include/qgtc.h, "Edge values"):
``values`` is a float32 [nnz] vector with one element per stored cell, in SLOT order - tile id, then tile row, then column ascending -
which depends on the tiles alone, so the same vector serves ``adj`` and ``adj.T``. :func:`edge_values` builds it from an edge list and
its weights, :func:`edge_slots` gives the slot of every edge of a list, :func:`edge_endpoints` the cell of every slot (for normalising
weights in torch: ``w * r[row] * c[col]``). ``out[i] = row_scale[i] * sum over j ascending of fl(values[slot(i, j)] * X[j])``: one
float32 multiply, then one add, never fused, as with ``src_scale``. :func:`tiledSDDMM` is the reverse primitive, one dot product per
stored cell, ``out[slot(i, j)] = DOT(A[i], B[j])`` with the attention's DOT; :func:`tiledAggregate` uses it for the gradient with respect
to the values, so a weighted aggregate is differentiable in X and in the weights, bit for bit the same on every run and without
atomics. ``edge_weight`` with ``src_scale``, ``edge_drop``, node masks, ``reduce="max"`` / ``"min"`` or ``attn`` is refused: not built.

:func:`tiledEdgeSoftmax` is the step between the two (include/qgtc.h, "Edge softmax"): it normalises a float32 [nnz] vector of per-edge
logits over each node's neighbourhood - a row's cells on ``adj``, a column's on ``adj.T`` - in one launch, with the attention's
exponential and the sum in ascending neighbour id, so forward and gradient are specified to the bit and use no atomics. A ``-inf``
logit masks its edge. :func:`tiledEdgeScores` is :func:`tiledSDDMM` under autograd (its two gradients are weighted products with the
incoming gradient as the weights), and :func:`tiledEdgeAttention` composes the three into dot-product attention over the edges,
``softmax(scale * Q K^T restricted to the edges) . V``, differentiable in Q, K and V. ``conv.TransformerConv`` is the layer on top.

All of that path takes HEADS without a loop (include/qgtc_heads.h): with ``heads=H`` the scores are float32 [nnz, H] (head-minor, the H
values of a cell adjacent), the softmax accepts and returns [nnz, H] with [n, H] statistics, ``edge_weight`` accepts [nnz, H] for an X
whose columns H divides, and ``tiledEdgeAttention(..., heads=H)`` is three launches forward and five backward for all heads - each head
bit for bit what the single-head call gives on its contiguous slice of columns.

:func:`tiledEdgeAdditiveScores` is the ADDITIVE score of GATv2 on the same path (include/qgtc_addscore.h): per stored cell and head,
``att . leaky_relu(own[o] + nbr[k])`` - the nonlinearity sits between the per-column add and the reduction, so it is neither a function
of two per-node scalars (``attn=``) nor a dot product (:func:`tiledSDDMM`). One launch gives the [nnz, H] scores, two give its
gradients, and :func:`tiledEdgeAdditiveAttention` composes it with the edge softmax and the weighted sum. ``conv.GATv2Conv`` is the
layer on top.

``fanout=(k, seed)`` on :func:`tiledMMFloat` and :func:`tiledAggregate` aggregates over a fixed-fanout sample - at most k neighbours per
output row, drawn inside the tile walk (include/qgtc_fanout.h): one selection launch gives a threshold per row, the aggregate then keeps
a cell when its hash reaches its row's threshold, and a backward on the other view looks the thresholds up per neighbour. The module
``fanout`` re-exports the sample (``sample_fanout``, ``FanoutSample``, defined here beside the other subgraphs of a call) and has the mini-batch
chain; the launches and their allocations are the family launchers' below. ``sage.SAGEConv`` is the layer on top.
A sample taken under node masks (``fanout.sample_fanout(view, k, seed, row_mask=, nbr_mask=)``; include/qgtc_blocks.h) carries them, and
``fanout=`` then runs on the induced subgraph: mini-batch GraphSAGE (``fanout.frontier``, ``fanout.sample_blocks``, ``SAGEConv(block=)``).
"""
from __future__ import annotations

import ctypes
import math
from typing import NamedTuple

import torch

from . import cabi, load_ext

_ext = load_ext()


# libqgtc_hip.so through ctypes, every signature from include/qgtc.h, for the entries the extension does not bind: qgtc_node_bitmap,
# qgtc_tiled_inv_degree and the edge-value index, SDDMM and edge-softmax entries. Loaded on first use; the extension has loaded the same
# library already.
_c_abi = cabi.load


def _c_call(what: str, on: torch.Tensor, fn, *args) -> None:
    """One C entry on ``torch.cuda.current_stream()`` of the operand's device (the stream handle is the entry's last argument): it
    enqueues and returns, like the extension's own calls, and can be captured into a graph."""
    if not on.is_cuda:
        raise ValueError(f"{what} needs its operand on a GPU, not on {on.device}")
    with torch.cuda.device(on.device):
        rc = fn(*args, ctypes.c_void_p(torch.cuda.current_stream(on.device).cuda_stream))
    if rc != 0:
        raise RuntimeError(f"{what}: {_c_abi().qgtc_strerror(rc).decode()} (rc {rc})")


def _inv_degree(deg: torch.Tensor) -> torch.Tensor:
    """float32 [n] = 1 / deg, correctly rounded, 0 where deg is 0: the reciprocal kernel of the degrees alone (qgtc_tiled_inv_degree)."""
    deg = deg.contiguous()
    out = torch.empty(deg.numel(), dtype=torch.float32, device=deg.device)
    _c_call("the reciprocal of the degrees", deg, _c_abi().qgtc_tiled_inv_degree, deg.data_ptr(), deg.numel(), out.data_ptr())
    return out

__all__ = ["TiledAdjacency", "pack_edges_tiled", "reorder_nodes", "tiledMM2Bit", "tiledMM2Int", "tiledMMFloat", "tiledAggregate",
           "add_self_loops", "node_bitmap", "edge_slots", "edge_endpoints", "edge_values", "tiledSDDMM", "tiledEdgeSoftmax",
           "tiledEdgeScores", "tiledEdgeAttention", "tiledEdgeAdditiveScores", "tiledEdgeAdditiveAttention"]


class TiledAdjacency:
    """One-plane n x n adjacency as its occupied tiles (device tensors):

    ``row_ptr`` int64 [S32(n) + 1]: the tiles of 32-row block rb are ``row_ptr[rb] .. row_ptr[rb+1] - 1``;
    ``kquad`` int32 [T]: the 128-column group of each tile, strictly ascending within a row block;
    ``tiles`` int32 words [T, 32, 4]: row r of the block, the tile's 4 words of that row (element i at word i>>5, bit 31-(i&31)).

    From ``pack_edges_tiled(..., reorder=True)`` the adjacency is that of the renumbered graph: ``perm`` int64 [n] (perm[new] = old)
    and ``rank`` int64 [n] (rank[old] = new) are set, and tiledMM2Bit / tiledMM2Int read X and give their output in the new
    numbering (:meth:`to_new`, :meth:`to_old`, :meth:`to_old_packed` move tensors across). Otherwise both are None and the node ids
    are the edge list's.

    :attr:`T` is the transposed adjacency (``transposed`` True): it shares the four tensors above, so nothing is copied, and adds
    the column index ``col_ptr`` int64 [S128(n) + 1] (the tiles of k-quad q are entries ``col_ptr[q] .. col_ptr[q+1] - 1``),
    ``col_tile`` int64 [T] (tile ids, ascending within a k-quad) and ``col_rb`` int32 [T] (each listed tile's row block), built by
    one device call on first use and cached on this object. ``adj.T.T is adj``; both share one numbering.
    """

    def __init__(self, n: int, row_ptr: torch.Tensor, kquad: torch.Tensor, tiles: torch.Tensor, perm: torch.Tensor | None = None,
                 rank: torch.Tensor | None = None):
        self.n = int(n)
        self.mask_words = _mask_words(self.n)   # the int32 words of a node bitmap of this graph
        self.row_ptr, self.kquad, self.tiles = row_ptr, kquad, tiles
        self.perm, self.rank = perm, rank
        self.transposed = False
        self._max_block_tiles = None
        self._other = None   # the transposed view (built on first use), or, on that view, the adjacency it transposes
        self._degrees = None  # [out_deg, in_deg, out_inv, in_inv], kept on the untransposed adjacency for both views
        self._sym = None      # [out, in] inverse square roots of the degrees, beside them
        self._val_index = None  # (val_ptr, val_row, nnz) of the edge values, kept on the untransposed adjacency for both views
        self._endpoints = None  # (row, col) of every slot, beside it

    @property
    def T(self) -> "TiledAdjacency":
        """The transposed adjacency A^T: tiledMM2Bit / tiledMM2Int on it sum over in-neighbours. Cached; ``adj.T.T is adj``."""
        if self._other is None:
            col_ptr, col_tile, col_rb = _ext._tiled_colindex(self.row_ptr, self.kquad, self.n)
            t = TiledAdjacency(self.n, self.row_ptr, self.kquad, self.tiles, self.perm, self.rank)
            t.transposed = True
            t.col_ptr, t.col_tile, t.col_rb = col_ptr, col_tile, col_rb
            t._other, self._other = self, t
        return self._other

    @property
    def n_tiles(self) -> int:
        return int(self.kquad.numel())

    @property
    def device(self) -> torch.device:
        return self.row_ptr.device

    @property
    def nbytes(self) -> int:
        """Bytes of the three tensors (512 a tile, 4 a k-quad index, 8 a row block); transposed, also of the column index (8 a
        k-quad, 12 a tile)."""
        parts = (self.row_ptr, self.kquad, self.tiles) + ((self.col_ptr, self.col_tile, self.col_rb) if self.transposed else ())
        return sum(t.numel() * t.element_size() for t in parts)

    @property
    def max_block_tiles(self) -> int:
        """Most tiles in one 32-row block; transposed, in one k-quad's list (one host read, on first use)."""
        if self._max_block_tiles is None:
            ptr = self.col_ptr if self.transposed else self.row_ptr
            self._max_block_tiles = int((ptr[1:] - ptr[:-1]).max().item()) if ptr.numel() > 1 else 0
        return self._max_block_tiles

    def _degree_tensors(self):
        base = _base(self)
        if base._degrees is None:
            base._degrees = _ext._tiled_degrees(base.row_ptr, base.kquad, base.tiles, base.n)
        return base._degrees

    def _masked_degrees(self, row_mask, nbr_mask) -> torch.Tensor:
        """int32 [n]: the terms the masked sum on this view adds per row - one masked N = 1 launch on a column of ones (exact: a degree
        is at most 2^23). Not cached."""
        ones = torch.ones((self.n, 1), dtype=torch.float32, device=self.device)
        return tiledMMFloat(self, ones, row_mask=row_mask, nbr_mask=nbr_mask).reshape(self.n).to(torch.int32)

    def degrees(self, row_mask: torch.Tensor | None = None, nbr_mask: torch.Tensor | None = None) -> torch.Tensor:
        """int32 [n]: the set cells in every row of this view - the out-degree on ``adj``, the in-degree on ``adj.T`` -, which is the
        number of terms tiledMM2Int sums for that row (cells of multiplicity 2 are unset and do not count; self loops do). In the
        adjacency's numbering (:meth:`to_old` moves it). One device call computes both directions on first use; ``adj`` and
        ``adj.T`` share the result.

        With ``row_mask`` / ``nbr_mask`` (bitmaps of :func:`node_bitmap`, relative to this view, or None = all nodes) the degrees of the
        masked graph: the neighbours in ``nbr_mask`` of every row in ``row_mask``, 0 for the other rows - what the unmasked method
        gives on ``pack_edges_tiled`` of the edges between the two sets. One masked N = 1 launch on a column of ones, not cached."""
        if row_mask is not None or nbr_mask is not None:
            return self._masked_degrees(row_mask, nbr_mask)
        return self._degree_tensors()[1 if self.transposed else 0]

    def mean_scale(self, row_mask: torch.Tensor | None = None, nbr_mask: torch.Tensor | None = None) -> torch.Tensor:
        """float32 [n]: 1 / degrees(), correctly rounded, 0 where the degree is 0 - the ``row_scale`` that turns tiledMM2Bit /
        tiledMM2Int on this view into the mean over neighbours. With ``row_mask`` / ``nbr_mask`` the masked graph's (as in
        :meth:`degrees`; not cached; the reciprocal is the same kernel's)."""
        if row_mask is not None or nbr_mask is not None:
            return _inv_degree(self._masked_degrees(row_mask, nbr_mask))
        return self._degree_tensors()[3 if self.transposed else 2]

    def sym_scale(self, row_mask: torch.Tensor | None = None, nbr_mask: torch.Tensor | None = None) -> torch.Tensor:
        """float32 [n]: 1 / sqrt(degrees()) of this view, both operations correctly rounded, 0 where the degree is 0. With
        ``row_scale=adj.sym_scale(), src_scale=adj.T.sym_scale()`` tiledMMFloat / tiledAggregate on ``adj`` give
        D_out^-1/2 . A . D_in^-1/2 (on ``adj.T`` swap the two views): on a symmetric edge list the GCN normalisation
        D^-1/2 . A . D^-1/2. Computed for both directions on first use; ``adj`` and ``adj.T`` share the result. With ``row_mask`` /
        ``nbr_mask`` the masked graph's (as in :meth:`degrees`; not cached; the same inverse-square-root kernel)."""
        if row_mask is not None or nbr_mask is not None:
            return _ext._tiled_inv_sqrt_degree(self._masked_degrees(row_mask, nbr_mask))
        base = _base(self)
        if base._sym is None:
            deg = self._degree_tensors()
            base._sym = [_ext._tiled_inv_sqrt_degree(deg[0]), _ext._tiled_inv_sqrt_degree(deg[1])]
        return base._sym[1 if self.transposed else 0]

    def to_rows(self) -> torch.Tensor:
        """The dense rows-layout words [PAD8(n), S128(n)*4] (what ``pack_edges(src, dst, n, n, 1)`` returns; transposed, what
        ``pack_edges(dst, src, n, n, 1)`` returns). A test aid for small n."""
        if self.transposed:
            n, p8, w = self.n, (self.n + 7) // 8 * 8, self.mask_words
            shifts = 31 - torch.arange(32, device=self.device, dtype=torch.int64)
            bits = (self._other.to_rows().to(torch.int64)[:, :, None] >> shifts) & 1            # [P8, W, 32]
            dense = torch.zeros((p8, w * 32), dtype=torch.int64, device=self.device)
            dense[:n, :n] = bits.reshape(p8, w * 32)[:n, :n].t()
            return (dense.view(p8, w, 32) << shifts).sum(-1).to(torch.int32).contiguous()
        n = self.n
        nrb, nq = (n + 31) // 32, (n + 127) // 128
        dense = torch.zeros((nrb * 32, nq, 4), dtype=torch.int32, device=self.device)
        if self.n_tiles:
            rb = torch.repeat_interleave(torch.arange(nrb, device=self.device), self.row_ptr[1:] - self.row_ptr[:-1])
            rows = rb[:, None] * 32 + torch.arange(32, device=self.device)[None, :]
            dense[rows, self.kquad.long()[:, None].expand(-1, 32)] = self.tiles
        return dense[: (n + 7) // 8 * 8].reshape((n + 7) // 8 * 8, nq * 4).contiguous()

    def to_new(self, x: torch.Tensor) -> torch.Tensor:
        """Rows of x [n, ...] in the edge list's numbering -> the adjacency's (x[perm]); x itself when not reordered."""
        if self.perm is None:
            return x
        assert x.size(0) == self.n, "x must have one row per node"
        return x.index_select(0, self.perm)

    def to_old(self, y: torch.Tensor) -> torch.Tensor:
        """Rows of y [n, ...] in the adjacency's numbering (a tiledMM2Int output) -> the edge list's (y[rank]); y itself when not
        reordered."""
        if self.rank is None:
            return y
        assert y.size(0) == self.n, "y must have one row per node"
        return y.index_select(0, self.rank)

    def to_old_packed(self, words: torch.Tensor, planes: int) -> torch.Tensor:
        """A rows-layout bit output [planes * PAD8(n), W] in the adjacency's numbering (tiledMM2Bit with output_bit = planes) ->
        the edge list's: rows 0 .. n-1 of every plane gathered by rank, the pad rows kept. ``words`` itself when not reordered."""
        if self.rank is None:
            return words
        p8 = (self.n + 7) // 8 * 8
        assert words.dim() == 2 and words.size(0) == planes * p8, "words must be [planes * PAD8(n), W]"
        v = words.view(planes, p8, words.size(1))
        out = v.clone()
        out[:, : self.n] = v.index_select(1, self.rank)
        return out.view_as(words)

    def __repr__(self) -> str:
        return (f"TiledAdjacency(n={self.n}, n_tiles={self.n_tiles}, nbytes={self.nbytes}, reordered={self.perm is not None}, "
                f"transposed={self.transposed})")


def _base(adj: TiledAdjacency) -> TiledAdjacency:
    """The untransposed adjacency of either view: the owner of what both views share."""
    return adj._other if adj.transposed else adj


def _mask_words(n: int) -> int:
    """S128(n) * 4: the int32 words of a node bitmap, and of one row of the dense rows layout."""
    return (n + 127) // 128 * 4


def _to_new_ids(rank: torch.Tensor, n: int, src: torch.Tensor, dst: torch.Tensor):
    """(src, dst) of an edge list moved to the numbering of ``rank``; out-of-range ids stay out of range (the packer and the slot search
    skip them)."""
    ok_s, ok_d = (src >= 0) & (src < n), (dst >= 0) & (dst < n)
    return torch.where(ok_s, rank.index_select(0, src.clamp(0, n - 1)), src), torch.where(ok_d, rank.index_select(0, dst.clamp(0, n - 1)), dst)


def reorder_nodes(src: torch.Tensor, dst: torch.Tensor, n: int, sweeps: int = 20, cap: int = 128, validate: bool = True) -> torch.Tensor:
    """perm (int64 [n] on the edges' device, perm[new] = old): a numbering under which neighbours have nearby ids, from size-capped
    label propagation on the symmetrised graph (``sweeps`` 0 .. 64, communities of about ``cap`` nodes; include/qgtc.h,
    "Node reordering"). Deterministic. ``validate`` raises on an out-of-range or negative index; without it such edges are skipped."""
    perm, _ = _ext._reorder_nodes(src, dst, int(n), int(sweeps), int(cap), bool(validate))
    return perm


def pack_edges_tiled(src: torch.Tensor, dst: torch.Tensor, n: int, validate: bool = True, reorder: bool = False) -> TiledAdjacency:
    """Tile-compressed adjacency of the raw edge list (src[i] -> row, dst[i] -> column; duplicates allowed: multiplicities
    1, 2, >= 3 quantise to 1, 0, 1 as in ``pack_edges``). ``validate`` raises on an out-of-range or negative index;
    without it such edges are skipped. ``reorder`` renumbers the nodes first (:func:`reorder_nodes` with its defaults) and packs
    the edges (rank[src], rank[dst]): the result carries ``perm`` / ``rank`` and works in the new numbering."""
    if not reorder:
        row_ptr, kquad, tiles = _ext._tiled_pack(src, dst, int(n), bool(validate))
        return TiledAdjacency(n, row_ptr, kquad, tiles)
    perm, rank = _ext._reorder_nodes(src, dst, int(n), 20, 128, bool(validate))
    if src.numel():
        src, dst = _to_new_ids(rank, n, src, dst)
    row_ptr, kquad, tiles = _ext._tiled_pack(src.contiguous(), dst.contiguous(), int(n), False)
    return TiledAdjacency(n, row_ptr, kquad, tiles, perm, rank)


def _check(adj) -> None:
    if not isinstance(adj, TiledAdjacency):
        raise TypeError("adj must be a TiledAdjacency (QGTC.pack_edges_tiled)")


def _check_scale(adj: TiledAdjacency, row_scale, name: str = "row_scale") -> None:
    if not isinstance(row_scale, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor (float32 [n]) or None")
    if row_scale.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, not {row_scale.dtype}")
    if row_scale.dim() != 1 or row_scale.numel() != adj.n:
        raise ValueError(f"{name} must have shape [{adj.n}], not {list(row_scale.shape)}")
    if row_scale.device != adj.device:
        raise ValueError(f"{name} must be on the adjacency's device {adj.device}, not {row_scale.device}")
    if not row_scale.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


_ON_T = {"_tiled_mm": "_tiled_mm_t", "_tiled_mm_f32": "_tiled_mm_f32_t", "_tiled_mm_f32_src": "_tiled_mm_f32_t_src"}


def _call(adj: TiledAdjacency, name: str, *args, **kw):
    """The binding ``name`` on the view of ``adj``: ``name`` itself after (row_ptr, kquad, tiles, n) or, on ``adj.T``, its twin of
    ``_ON_T`` after (col_ptr, col_tile, col_rb, tiles, n). The one place that tells the views apart for the extension. Without a
    keyword the binding gets no keyword dictionary at all: pybind11 searches a dictionary, even an empty one, for every argument left
    to its default."""
    if adj.transposed:
        fn, view = getattr(_ext, _ON_T[name]), (adj.col_ptr, adj.col_tile, adj.col_rb, adj.tiles, adj.n)
    else:
        fn, view = getattr(_ext, name), (adj.row_ptr, adj.kquad, adj.tiles, adj.n)
    return fn(*view, *args, **kw) if kw else fn(*view, *args)


def _tiled(adj: TiledAdjacency, bit_X: torch.Tensor, N: int, bit2: int, output_bit: int, to_float: bool, row_scale,
           row_mask=None, nbr_mask=None) -> torch.Tensor:
    _check(adj)
    if row_mask is not None or nbr_mask is not None:
        # the masked entries of include/qgtc_bitnodes.h, through ctypes: tiled_bit allocates the output and launches
        from . import tiled_bit

        if row_scale is not None:
            _check_scale(adj, row_scale)
        return tiled_bit.masked(adj, bit_X, N, bit2, output_bit, to_float, row_scale, row_mask, nbr_mask)
    if row_scale is None:
        # exactly the unscaled call
        return _call(adj, "_tiled_mm", bit_X, int(N), int(bit2), int(output_bit), to_float)
    _check_scale(adj, row_scale)
    return _call(adj, "_tiled_mm", bit_X, int(N), int(bit2), int(output_bit), to_float, row_scale)


def tiledMM2Bit(adj: TiledAdjacency, bit_X: torch.Tensor, N: int, bit2: int, output_bit: int,
                row_scale: torch.Tensor | None = None, row_mask: torch.Tensor | None = None,
                nbr_mask: torch.Tensor | None = None) -> torch.Tensor:
    """requant(A . X) in the rows layout [output_bit * PAD8(n), S128(N)*4]: ``bitMM2Bit(A_rows, bit_X, n, n, N, 1, bit2,
    output_bit)``. bit_X: cols layout [bit2][PAD128(N)][S128(n)*4] (``val2bit(X, bit2, True, False)`` / ``bitMM2Bit_col``).
    On ``adj.T`` it is requant(A^T . X), from the same tiles, bit-transposed in the kernel.

    With ``row_scale`` (float32 [n], contiguous, on the adjacency's device, in the adjacency's numbering like bit_X) the words hold
    the value quantiser of y = float(A . X) * row_scale[:, None] instead: ``val2bit(tiledMM2Int(adj, bit_X, N, bit2, row_scale),
    output_bit, False, False)``, word for word, in one kernel.

    With ``row_mask`` / ``nbr_mask`` (bitmaps of :func:`node_bitmap` relative to this view, or None = all nodes; include/qgtc_bitnodes.h)
    the product runs on the induced subgraph, in one launch and without packing a second adjacency: a row outside ``row_mask`` holds what a
    row without neighbours holds, a neighbour outside ``nbr_mask`` is never read, a block of 32 rows (128 on ``adj.T``) without a live row
    reads no tile, and the words are those of the unmasked call on ``pack_edges_tiled`` of the edges between the two sets. With both None
    the call is the one it always was. The masked calls go through ctypes on the current stream and can be captured. Measured on the
    reordered arxiv- and reddit-sized graphs at N = 64: a contiguous or community-aligned eighth of the nodes
    as both masks runs at 0.05 - 0.39 of the plain launch and 0.06 - 0.37 of the filter-and-re-pack route; a random eighth leaves every
    block live and costs 0.64 - 1.27 of the plain launch and up to 2.2x the re-pack route; all-ones masks cost 0.78 - 1.42 of it."""
    return _tiled(adj, bit_X, N, bit2, output_bit, False, row_scale, row_mask, nbr_mask)


def tiledMM2Int(adj: TiledAdjacency, bit_X: torch.Tensor, N: int, bit2: int, row_scale: torch.Tensor | None = None,
                row_mask: torch.Tensor | None = None, nbr_mask: torch.Tensor | None = None) -> torch.Tensor:
    """float32 [n, N] = A . X: ``bitMM2Int(A_rows, bit_X, n, n, N, 1, bit2, True)``; on ``adj.T``, A^T . X. With ``row_scale`` every
    row r is multiplied by row_scale[r] (one float32 multiply of the exact sum's float32 conversion). ``row_mask`` / ``nbr_mask`` as in
    :func:`tiledMM2Bit`: a row outside ``row_mask`` is +0 (times its ``row_scale``)."""
    return _tiled(adj, bit_X, N, bit2, 1, True, row_scale, row_mask, nbr_mask)


def _check_float_operand(adj: TiledAdjacency, X) -> None:
    if not isinstance(X, torch.Tensor):
        raise TypeError(f"X must be a torch.Tensor (float32 [{adj.n}, N]), not {type(X).__name__}")
    if X.dtype != torch.float32:
        raise TypeError(f"X must be float32, not {X.dtype}")
    if X.dim() != 2 or X.size(0) != adj.n or X.size(1) < 1:
        raise ValueError(f"X must have shape [{adj.n}, N] with N >= 1, not {list(X.shape)}")
    if X.device != adj.device:
        raise ValueError(f"X must be on the adjacency's device {adj.device}, not {X.device}")
    if not X.is_contiguous():
        raise ValueError(f"X must be contiguous; its strides are {list(X.stride())}")


def _check_slope(negative_slope) -> float:
    slope = float(negative_slope)
    if not 0.0 <= slope <= 1.0:   # a NaN fails both comparisons
        raise ValueError(f"negative_slope must lie in [0, 1], not {negative_slope!r}")
    return slope


def _attn_heads(adj: TiledAdjacency, score) -> int:
    """H when ``score`` is a per-head score [n, H] with H at least 2, otherwise 0: the score is then checked as the vector [n] it
    always had to be ([n, 1] included, which stays refused)."""
    return score.size(1) if isinstance(score, torch.Tensor) and score.dim() == 2 and score.size(0) == adj.n and score.size(1) >= 2 else 0


def _check_attn(adj: TiledAdjacency, attn, X=None) -> tuple[torch.Tensor, torch.Tensor]:
    if not isinstance(attn, (tuple, list)) or len(attn) != 2:
        raise TypeError("attn must be a pair (att_out, att_nbr) of float32 [n] tensors")
    H = _attn_heads(adj, attn[0]) or _attn_heads(adj, attn[1])
    if H == 0:
        _check_scale(adj, attn[0], "att_out")
        _check_scale(adj, attn[1], "att_nbr")
        return attn[0], attn[1]
    # scores per head: float32 [n, H], head-minor, both of one shape, H a divisor of X's columns
    for name, t in (("att_out", attn[0]), ("att_nbr", attn[1])):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor (float32 [n] or [n, H])")
        if t.dtype != torch.float32:
            raise TypeError(f"{name} must be float32, not {t.dtype}")
        if tuple(t.shape) != (adj.n, H):
            raise ValueError(f"att_out and att_nbr must have the same shape [{adj.n}, {H}], not {list(attn[0].shape)} and {list(attn[1].shape)}")
        if t.device != adj.device:
            raise ValueError(f"{name} must be on the adjacency's device {adj.device}, not {t.device}")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    if isinstance(X, torch.Tensor) and X.dim() == 2 and X.size(1) % H != 0:
        raise ValueError(f"attn has {H} heads, which do not divide X's {X.size(1)} columns")
    return attn[0], attn[1]


def _edge_drop_key(edge_drop):
    """None, or (threshold, seed) of include/qgtc.h, "Edge dropout", from ``edge_drop=(rate, seed)``: threshold = floor(rate * 2^32)
    computed in double. A non-pair or a seed that is no int is a TypeError; a rate outside [0, 1) or NaN and a seed outside [0, 2^64)
    are a ValueError."""
    if edge_drop is None:
        return None
    if not isinstance(edge_drop, (tuple, list)) or len(edge_drop) != 2:
        raise TypeError("edge_drop must be a pair (rate, seed) or None")
    rate, seed = edge_drop
    if isinstance(rate, bool) or not isinstance(rate, (int, float)):
        raise TypeError(f"edge_drop's rate must be a float in [0, 1), not {type(rate).__name__}")
    if isinstance(seed, bool) or not isinstance(seed, int):
        raise TypeError(f"edge_drop's seed must be an int in [0, 2^64), not {type(seed).__name__}")
    rate = float(rate)
    if not 0.0 <= rate < 1.0:   # a NaN fails both comparisons
        raise ValueError(f"edge_drop's rate must lie in [0, 1), not {rate!r}")
    if not 0 <= seed < (1 << 64):
        raise ValueError(f"edge_drop's seed must lie in [0, 2^64), not {seed!r}")
    return int(math.floor(rate * 4294967296.0)), seed


def node_bitmap(nodes: torch.Tensor, n: int) -> torch.Tensor:
    """int32 [S128(n) * 4]: the bitmap of a node set (include/qgtc.h, "Node masks"; node i at word i >> 5, bit 31 - (i & 31), pad bits
    zero), on the device of ``nodes`` (a GPU), built by one small kernel on the current stream (the C entry qgtc_node_bitmap, called
    through ctypes: the extension binds no new name for it). ``nodes`` is a bool [n] tensor, or an int64 tensor of node ids in any
    order, duplicates allowed; an id outside 0 .. n - 1 is a ValueError (one host read), any other dtype a TypeError. The ids are the
    ADJACENCY'S: on a reordered adjacency move a bool mask over with ``adj.to_new(mask)`` first (an id list i becomes
    ``adj.rank[i]``)."""
    n = int(n)
    if not isinstance(nodes, torch.Tensor):
        raise TypeError(f"nodes must be a torch.Tensor (bool [n] or int64 ids), not {type(nodes).__name__}")
    if not 1 <= n <= (1 << 23):
        raise ValueError(f"n must lie in [1, 2^23], not {n}")
    if nodes.dtype == torch.bool:
        if nodes.dim() != 1 or nodes.numel() != n:
            raise ValueError(f"a bool nodes must have shape [{n}], not {list(nodes.shape)}")
        flags = nodes.contiguous()
    elif nodes.dtype == torch.int64:
        if nodes.dim() != 1:
            raise ValueError(f"an id list must have one dimension, not {nodes.dim()}")
        if nodes.numel() and not bool(((nodes >= 0) & (nodes < n)).all()):
            raise ValueError(f"nodes holds an id outside 0 .. {n - 1}")
        flags = torch.zeros(n, dtype=torch.bool, device=nodes.device)
        flags[nodes] = True   # duplicates write the same value
    else:
        raise TypeError(f"nodes must be bool or int64, not {nodes.dtype}")
    out = torch.empty(_mask_words(n), dtype=torch.int32, device=flags.device)
    _c_call("node_bitmap", flags, _c_abi().qgtc_node_bitmap, flags.data_ptr(), n, out.data_ptr(), out.numel())
    return out


def _check_mask(adj: TiledAdjacency, mask, name: str) -> None:
    if not isinstance(mask, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor (the int32 bitmap of tiled.node_bitmap) or None")
    if mask.dtype != torch.int32:
        raise TypeError(f"{name} must be int32 (tiled.node_bitmap), not {mask.dtype}")
    words = adj.mask_words
    if mask.dim() != 1 or mask.numel() != words:
        raise ValueError(f"{name} must have shape [{words}] (S128(n) * 4 words), not {list(mask.shape)}")
    if mask.device != adj.device:
        raise ValueError(f"{name} must be on the adjacency's device {adj.device}, not {mask.device}")
    if not mask.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def _check_k_seed(k, seed) -> None:
    if isinstance(k, bool) or not isinstance(k, int):
        raise TypeError(f"fanout's k must be an int >= 1, not {type(k).__name__}")
    if isinstance(seed, bool) or not isinstance(seed, int):
        raise TypeError(f"fanout's seed must be an int in [0, 2^64), not {type(seed).__name__}")
    if k < 1:
        raise ValueError(f"fanout's k must be at least 1, not {k!r}")
    if not 0 <= seed < (1 << 64):
        raise ValueError(f"fanout's seed must lie in [0, 2^64), not {seed!r}")


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
            return _inv_degree(self.counts)
        if _masked(self):
            raise ValueError("a masked FanoutSample needs its counts for the mean (sample_fanout returns them)")
        return _inv_degree(self.view.degrees().clamp(max=min(self.k, (1 << 31) - 1)))

    def __repr__(self) -> str:
        masks = "".join(f", {name}" for name, m in (("row_mask", self.row_mask), ("nbr_mask", self.nbr_mask)) if m is not None)
        return (f"FanoutSample(k={self.k}, seed={self.seed:#x}, axis={'columns' if self.view.transposed else 'rows'}, "
                f"n={self.view.n}{masks})")


def check_fanout(adj: TiledAdjacency, fanout) -> None:
    """The refusals of ``fanout=`` itself: a pair (k, seed) with k an int >= 1 and the seed under ``edge_drop``'s rules, or a
    :class:`FanoutSample` of this adjacency (either view). Anything else is a TypeError; a sample of another adjacency a ValueError."""
    if isinstance(fanout, FanoutSample):
        if not isinstance(fanout.view, TiledAdjacency) or _base(fanout.view) is not _base(adj):
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
                _check_mask(adj, getattr(fanout, name), f"a FanoutSample's {name}")
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


def _ptr(t):
    return None if t is None else t.data_ptr()


def _masked(of) -> bool:
    """Whether a subgraph, or a sample, carries a node bitmap."""
    return of.row_mask is not None or of.nbr_mask is not None


_NO_KW: dict = {}   # read only: ``**`` copies it, and ``_call`` hands pybind11 no dictionary when it is empty


class _Subgraph(NamedTuple):
    """The subgraph one call aggregates over, of exactly one kind: ALL nodes and edges (the one
    instance ``_ALL``: a plain call constructs nothing), edge dropout (``key``, the checked (threshold, seed)), node masks (``row_mask`` /
    ``nbr_mask``, relative to the view of the call, either may be None) or a :class:`FanoutSample` (which carries its own masks, relative
    to the view it was taken on). ``_resolve`` builds it once, through :meth:`of`; the launchers, the C tails and the backwards ask it,
    and nobody else tells the kinds apart. ``kw`` is what the extension's bindings take for it - no keyword, ``edge_drop=`` or
    ``node_masks=`` -, or None: a sample has no binding route; ``suffix`` is what the name of a C entry ends in for it. (Fields, not
    methods: every launch reads one of them.)"""
    key: tuple | None = None
    row_mask: torch.Tensor | None = None
    nbr_mask: torch.Tensor | None = None
    sample: FanoutSample | None = None
    kw: dict | None = _NO_KW
    suffix: str = ""

    @classmethod
    def of(cls, key=None, row_mask=None, nbr_mask=None, sample=None) -> "_Subgraph":
        """The subgraph of checked arguments, at most one kind of which is set; the one place that writes ``kw`` and ``suffix``. (The
        fields are passed by position: a NamedTuple takes keywords at half again the cost, on every masked call.)"""
        if sample is not None:
            return cls(None, None, None, sample, None, "_fanout_nodes" if _masked(sample) else "_fanout")
        if key is not None:
            return cls(key, None, None, None, {"edge_drop": key}, "_drop")
        if row_mask is None and nbr_mask is None:
            return _ALL
        return cls(None, row_mask, nbr_mask, None, {"node_masks": (row_mask, nbr_mask)}, "_nodes")

    def c_tail(self, adj: TiledAdjacency) -> tuple:
        """The trailing arguments of a C entry on the view of ``adj``. A key is (threshold, seed); node masks are (row_mask, nbr_mask,
        mask_words). A sample is (thr, thr_of_nbr, seed): OWN (0) on the view it was taken on, NBR (1) on the other - check_fanout has made
        sure that both views belong to one adjacency, so their direction alone tells them apart - and a masked sample adds its bitmaps
        relative to the view walked: its own on its own view, the two swapped on the other."""
        if self is _ALL:
            return ()
        if self.key is not None:
            return tuple(self.key)
        s = self.sample
        if s is None:
            return _ptr(self.row_mask), _ptr(self.nbr_mask), adj.mask_words
        nbr = int(s.view.transposed != adj.transposed)
        tail = (s.thr.data_ptr(), nbr, s.seed)
        if _masked(s):
            row, other = (s.nbr_mask, s.row_mask) if nbr else (s.row_mask, s.nbr_mask)
            tail += (_ptr(row), _ptr(other), adj.mask_words)
        return tail

    def other(self) -> "_Subgraph":
        """Itself as the other view sees it - what every backward needs: node masks swapped (a neighbour there is an output row
        here); a key and a sample unchanged (both name cells of the adjacency, and ``c_tail`` reads a sample per view)."""
        if self.row_mask is None and self.nbr_mask is None:
            return self
        return self.of(row_mask=self.nbr_mask, nbr_mask=self.row_mask)

    def tensors(self) -> tuple:
        """Its tensors, for ``save_for_backward`` (None where it has none): every tensor a backward reads goes through there - a
        reference, nothing is copied -, so that autograd's version check sees an in-place edit between the forward and the backward and
        raises instead of differentiating another graph."""
        s = self.sample
        return (self.row_mask, self.nbr_mask) if s is None else (s.thr, s.row_mask, s.nbr_mask, s.counts)

    def rebuilt(self, tensors) -> "_Subgraph":
        """Itself in a backward, from the saved (version-checked) ``tensors()``."""
        s = self.sample
        if s is not None:
            return self.of(sample=FanoutSample(s.view, s.k, s.seed, *tensors))
        if self.row_mask is None and self.nbr_mask is None:
            return self
        return self.of(row_mask=tensors[0], nbr_mask=tensors[1])


_ALL = _Subgraph()


def _view_args(adj: TiledAdjacency) -> tuple:
    """(the view's index pointers, tiles, n_tiles, n) as every C entry takes them first; an adjacency without tiles passes NULL
    pointers. The one place that turns a view into pointer arguments."""
    T = adj.n_tiles
    view = (adj.col_ptr, adj.col_tile, adj.col_rb, adj.tiles) if adj.transposed else (adj.row_ptr, adj.kquad, adj.tiles)
    return tuple(t.data_ptr() if T else None for t in view) + (T, adj.n)


def _c_name(stem: str, heads, transposed: bool, sub: _Subgraph = _ALL) -> str:
    """The name of the C entry of a family: ``stem`` (the plain single-head entry of the row view, ending in ``_f32`` where it has
    heads), ``_heads`` before that ending for the entry with heads, ``_t`` on ``adj.T``, then the subgraph's suffix. The one place
    that composes a name; it opens no library."""
    if heads:
        stem = stem[:-len("_f32")] + "_heads_f32"
    return stem + ("_t" if transposed else "") + sub.suffix


def _c_entry(stem: str, heads, adj: TiledAdjacency, sub: _Subgraph = _ALL):
    return getattr(_c_abi(), _c_name(stem, heads, adj.transposed, sub))


def sample_fanout(adj_view: TiledAdjacency, k: int, seed: int, row_mask: torch.Tensor | None = None,
                  nbr_mask: torch.Tensor | None = None) -> FanoutSample:
    """The sample of fanout ``k`` under ``seed`` on the view passed (``adj``: at most k out-neighbours per row of A; ``adj.T``: at most k
    in-neighbours per column): one selection launch on the current stream, no host read. The sample is in the adjacency's own numbering
    (the new ids on a reordered adjacency).

    With ``row_mask`` and / or ``nbr_mask`` (bitmaps of ``tiled.node_bitmap``, relative to the view passed) the sample is taken on the
    induced subgraph: only the nodes of ``row_mask`` are sampled, among their neighbours in ``nbr_mask``; a node outside ``row_mask``
    keeps nothing and none of its tiles is read. Still one launch; the sample carries the masks and ``counts``. It is, word for word, the
    unmasked sample of ``pack_edges_tiled`` of the edges between the two sets."""
    _check(adj_view)
    _check_k_seed(k, seed)
    thr = torch.empty(adj_view.n, dtype=torch.int32, device=adj_view.device)
    if row_mask is None and nbr_mask is None:
        _c_call("the fanout selection", thr, _c_entry("qgtc_tiled_fanout_thr", False, adj_view), *_view_args(adj_view),
                min(k, (1 << 31) - 1), seed, thr.data_ptr(), thr.numel())
        return FanoutSample(adj_view, k, seed, thr)
    for name, mask in (("row_mask", row_mask), ("nbr_mask", nbr_mask)):
        if mask is not None:
            _check_mask(adj_view, mask, name)
    masks = _Subgraph.of(row_mask=row_mask, nbr_mask=nbr_mask)
    counts = torch.empty(adj_view.n, dtype=torch.int32, device=adj_view.device)
    _c_call("the masked fanout selection", thr, _c_entry("qgtc_tiled_fanout_thr", False, adj_view, masks), *_view_args(adj_view),
            min(k, (1 << 31) - 1), seed, thr.data_ptr(), thr.numel(), counts.data_ptr(), counts.numel(), *masks.c_tail(adj_view))
    return FanoutSample(adj_view, k, seed, thr, row_mask, nbr_mask, counts)


def as_sample(adj: TiledAdjacency, fanout) -> FanoutSample:
    """The checked ``fanout=`` as a sample: a pair is drawn on the view passed (one selection launch), a sample is itself."""
    check_fanout(adj, fanout)
    return fanout if isinstance(fanout, FanoutSample) else sample_fanout(adj, int(fanout[0]), int(fanout[1]))


def _value_index(adj: TiledAdjacency):
    """(val_ptr int64 [T + 1], val_row int16 [T, 32], nnz) of include/qgtc.h, "Edge values": one kernel for the tiles' bit counts and the
    in-tile row prefix, ``torch.cumsum`` for the scan, one host read for nnz. Built on first use and kept on the untransposed adjacency
    for both views."""
    base = _base(adj)
    if base._val_index is None:
        T = base.n_tiles
        counts = torch.empty(T, dtype=torch.int64, device=base.device)
        val_row = torch.empty((T, 32), dtype=torch.int16, device=base.device)
        if T:
            _c_call("the edge-value index", base.tiles, _c_abi().qgtc_tiled_value_index, base.tiles.data_ptr(), T, counts.data_ptr(),
                    val_row.data_ptr())
        val_ptr = torch.zeros(T + 1, dtype=torch.int64, device=base.device)
        if T:
            val_ptr[1:] = torch.cumsum(counts, 0)
        nnz = int(val_ptr[-1].item())
        if nnz >= (1 << 31):
            raise ValueError(f"the adjacency stores {nnz} cells: edge values are built for fewer than 2^31")
        base._val_index = (val_ptr, val_row, nnz)
    return base._val_index


def _check_edge_vector(adj: TiledAdjacency, values, name: str, X=None) -> None:
    """The checks of a per-edge vector, ``edge_weight`` or one of another name: float32 [nnz] in slot order, or [nnz, H] with a value
    per stored cell and head (H at least 2 and, for ``edge_weight``, a divisor of the columns of ``X``)."""
    weight = name == "edge_weight"
    if not isinstance(values, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor (float32 [nnz], " + ("tiled.edge_values) or None" if weight else "in slot order)"))
    if values.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, not {values.dtype}")
    if values.device != adj.device:
        raise ValueError(f"{name} must be on the adjacency's device {adj.device}, not {values.device}")
    nnz = _value_index(adj)[2]
    if values.dim() == 2 and values.size(0) == nnz and values.size(1) >= 2:   # [nnz, H]: a value per stored cell and head
        if isinstance(X, torch.Tensor) and X.dim() == 2 and X.size(1) % values.size(1) != 0:
            raise ValueError(f"{name} has {values.size(1)} heads, which do not divide X's {X.size(1)} columns")
    elif values.dim() != 1 or values.numel() != nnz:
        raise ValueError(f"{name} must have shape [{nnz}] (one value per stored cell)" + ("" if weight else f" or [{nnz}, H] with H >= 2") +
                         f", not {list(values.shape)}")
    if not values.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def _check_edge_weight(adj: TiledAdjacency, values, src_scale=None, key=None, masked: bool = False, reduce: str = "sum", attn=None,
                       X=None) -> None:
    """The refusals of ``edge_weight``: the combinations that are not built, then the vector itself."""
    for name, on in (("src_scale", src_scale is not None), ("edge_drop", key is not None), ("row_mask / nbr_mask", masked),
                     (f'reduce="{reduce}"', reduce != "sum"), ("attn", attn is not None)):
        if on:
            raise ValueError(f"edge_weight cannot be combined with {name}: not built")
    _check_edge_vector(adj, values, "edge_weight", X)


def edge_slots(adj: TiledAdjacency, src: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    """int64 [E]: the slot of the cell of every edge (src[e] -> dst[e]) of an edge list, -1 where the cell is not stored - the edge is
    not in the graph, multiplicity 2 quantised it to 0, or an id lies outside 0 .. n - 1 (include/qgtc.h, "Edge values"). ``src`` /
    ``dst`` are int64 [E] on the adjacency's device, in the EDGE LIST'S numbering with the row end first, whichever view ``adj`` is (on a
    reordered adjacency they are mapped through ``rank`` first). One kernel on the current stream: a binary search per edge."""
    _check(adj)
    base = _base(adj)
    for name, t in (("src", src), ("dst", dst)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != 1:
            raise TypeError(f"{name} must be a one-dimensional int64 torch.Tensor")
        if t.device != base.device:
            raise ValueError(f"{name} must be on the adjacency's device {base.device}, not {t.device}")
    if src.numel() != dst.numel():
        raise ValueError("src and dst must have the same length")
    n = base.n
    if base.rank is not None and src.numel():
        src, dst = _to_new_ids(base.rank, n, src, dst)
    src, dst = src.contiguous(), dst.contiguous()
    val_ptr, val_row, _ = _value_index(base)
    out = torch.empty(src.numel(), dtype=torch.int64, device=base.device)
    if src.numel():
        T = base.n_tiles
        _c_call("edge_slots", src, _c_abi().qgtc_tiled_edge_slots, base.row_ptr.data_ptr(), base.kquad.data_ptr() if T else None,
                base.tiles.data_ptr() if T else None, T, n, val_ptr.data_ptr(), val_row.data_ptr() if T else None, src.data_ptr(),
                dst.data_ptr(), src.numel(), out.data_ptr())
    return out


def edge_endpoints(adj: TiledAdjacency) -> tuple[torch.Tensor, torch.Tensor]:
    """(row, col), int32 [nnz] each: the cell of ``adj`` (untransposed, whichever view is passed) that every slot belongs to, in the
    ADJACENCY'S numbering (``adj.perm[row]`` gives the edge list's ids). For normalising weights in torch,
    ``values * r[row.long()] * c[col.long()]``. One kernel on first use; cached for both views."""
    _check(adj)
    base = _base(adj)
    if base._endpoints is None:
        val_ptr, val_row, nnz = _value_index(base)
        row = torch.empty(nnz, dtype=torch.int32, device=base.device)
        col = torch.empty(nnz, dtype=torch.int32, device=base.device)
        if nnz:
            _c_call("edge_endpoints", base.tiles, _c_abi().qgtc_tiled_edge_endpoints, base.row_ptr.data_ptr(), base.kquad.data_ptr(),
                    base.tiles.data_ptr(), base.n_tiles, base.n, val_ptr.data_ptr(), val_row.data_ptr(), row.data_ptr(), col.data_ptr(), nnz)
        base._endpoints = (row, col)
    return base._endpoints


def edge_values(adj: TiledAdjacency, src: torch.Tensor, dst: torch.Tensor, weight: torch.Tensor, validate: bool = True) -> torch.Tensor:
    """float32 [nnz]: the ``edge_weight`` vector of an edge list with one weight per edge - zeros with ``weight[e]`` written at the slot
    of edge e (:func:`edge_slots`; ids in the edge list's numbering). With ``validate`` (one host read, like
    ``pack_edges_tiled(validate=True)``) an edge without a stored cell, a cell named by two edges and a stored cell no edge names are
    each a ValueError; without it edges without a cell are skipped and which of two duplicates wins is unspecified."""
    if not isinstance(weight, torch.Tensor) or weight.dtype != torch.float32 or weight.dim() != 1:
        raise TypeError("weight must be a one-dimensional float32 torch.Tensor")
    slots = edge_slots(adj, src, dst)
    if weight.numel() != slots.numel():
        raise ValueError(f"weight must have one element per edge ({slots.numel()}), not {weight.numel()}")
    if weight.device != slots.device:
        raise ValueError(f"weight must be on the adjacency's device {slots.device}, not {weight.device}")
    nnz = _value_index(adj)[2]
    values = torch.zeros(nnz, dtype=torch.float32, device=slots.device)
    found = slots >= 0
    if validate:
        hits = torch.zeros(nnz, dtype=torch.int64, device=slots.device)
        hits.index_add_(0, slots[found], torch.ones_like(slots[found]))
        absent, dup, unnamed = (int(v) for v in torch.stack([(~found).sum(), (hits > 1).sum(), (hits == 0).sum()]).tolist())
        if absent:
            raise ValueError(f"{absent} edge(s) have no stored cell in the adjacency (absent, quantised to 0, or an id out of range)")
        if dup:
            raise ValueError(f"{dup} stored cell(s) are named by more than one edge")
        if unnamed:
            raise ValueError(f"{unnamed} stored cell(s) are named by no edge: every cell needs a weight")
    values[slots[found]] = weight[found]
    return values


def _check_heads(heads, width: int) -> int:
    """``heads`` as an int: at least 1 and a divisor of ``width``, the columns of the node matrices. Another value is a ValueError,
    another type a TypeError."""
    if isinstance(heads, bool) or not isinstance(heads, int):
        raise TypeError(f"heads must be an int, not {type(heads).__name__}")
    if heads < 1 or width % heads != 0:
        raise ValueError(f"heads must be at least 1 and divide the {width} columns, not {heads}")
    return heads


def _view_ptrs(adj: TiledAdjacency):
    """What every entry of include/qgtc_heads.h takes: ``_view_args`` first - and the pointers of the value index, which come later in
    the argument lists."""
    val_ptr, val_row, _ = _value_index(adj)
    T = adj.n_tiles
    return _view_args(adj), (val_ptr.data_ptr() if T else None, val_row.data_ptr() if T else None)


def _sddmm(base: TiledAdjacency, A: torch.Tensor, B: torch.Tensor, heads: int) -> torch.Tensor:
    """float32 [nnz, heads] of qgtc_tiled_sddmm_heads_f32 on the untransposed adjacency (the caller has swapped the operands of the
    other view): one launch on the current stream; one head is the single-head kernel."""
    nnz = _value_index(base)[2]
    out = torch.empty((nnz, heads), dtype=torch.float32, device=base.device)
    if nnz:
        head, idx = _view_ptrs(base)
        _c_call("tiledSDDMM", A, _c_abi().qgtc_tiled_sddmm_heads_f32, *head, A.data_ptr(), B.data_ptr(), A.numel(), A.size(1), *idx,
                out.data_ptr(), nnz, heads)
    return out


def tiledSDDMM(adj: TiledAdjacency, A: torch.Tensor, B: torch.Tensor, heads: int = 1) -> torch.Tensor:
    """float32 [nnz] in slot order: ``out[slot(i, j)] = DOT(A[i], B[j])`` for every stored cell (i, j) of this view - on ``adj`` row i of A
    with row j of B; on ``adj.T`` the cell is the same one of ``adj`` and the operands swap, so the same kernel runs. DOT is the
    attention's (include/qgtc.h, "Attention tiled products"): 64 strided partial sums, then the xor butterfly, every step one float32
    operation, so the result is the same bits on every launch. Each slot is written once, without atomics. A and B are float32 [n, N],
    contiguous, on the adjacency's device, in the adjacency's numbering. It is the gradient of a weighted aggregate for its weights, a
    link score, and the building block of dot-product attention.

    With ``heads=H`` > 1 (H dividing N; head h is the columns h d .. (h + 1) d - 1, d = N / H) the result is float32 [nnz, H],
    ``out[slot, h]`` the DOT of head h's columns: one launch for all heads (include/qgtc_heads.h), each head bit for bit the single-head
    call on its contiguous slice. ``heads=1`` is the call it always was. A ``heads`` that does not divide N is a ValueError."""
    _check(adj)
    _check_float_operand(adj, A)
    heads = _check_heads(heads, A.size(1))
    if not isinstance(B, torch.Tensor) or B.dtype != torch.float32:
        raise TypeError("B must be a float32 torch.Tensor")
    if B.shape != A.shape or B.device != A.device or not B.is_contiguous():
        raise ValueError(f"B must be contiguous, on A's device and of A's shape {list(A.shape)}, not {list(B.shape)}")
    if adj.transposed:
        A, B = B, A
    out = _sddmm(_base(adj), A, B, heads)
    return out if heads > 1 else out.view(-1)


# ---- one launcher per family: (adj, operands..., subgraph) -> freshly allocated outputs --------------------
def _c_route(heads, sub: _Subgraph) -> bool:
    """The route of one launch, chosen here for every family. False: the extension's binding, which takes one head under no mask,
    edge dropout or node masks. True: the C entry through ctypes, which takes heads and samples. Heads over a sample are not built:
    ``_resolve`` refuses them first, so that ValueError is never reached through a public call."""
    if sub.kw is not None:
        return bool(heads)
    if heads:
        raise ValueError("fanout cannot be combined with [n, H] scores: not built")
    return True


def _c_launch(what: str, on: torch.Tensor, stem: str, heads, adj: TiledAdjacency, sub: _Subgraph, *args) -> None:
    """One launch of the C entry of (``stem``, heads, the view, the subgraph): the view's arguments, the operands, ``heads`` where the
    entry has them, the subgraph's tail."""
    _c_call(f"the {what} with heads" if heads else f"the sampled {what}", on, getattr(_c_abi(), _c_name(stem, heads, adj.transposed, sub)),
            *_view_args(adj), *args, *((heads,) if heads else ()), *sub.c_tail(adj))


def _sum(adj: TiledAdjacency, X: torch.Tensor, row_scale, src_scale, sub: _Subgraph) -> torch.Tensor:
    """diag(row_scale) . A . diag(src_scale) . X over the subgraph, either scale optional: one launch."""
    if sub.kw is not None:   # _c_route(0, sub), inline: every plain call comes through here
        if src_scale is not None:
            return _call(adj, "_tiled_mm_f32_src", X, row_scale, src_scale, **sub.kw)
        return _call(adj, "_tiled_mm_f32", X, row_scale, **sub.kw)
    out = torch.empty_like(X)
    _c_launch("sum", X, "qgtc_tiledmm_f32", 0, adj, sub, X.data_ptr(), X.numel(), X.size(1), _ptr(row_scale), _ptr(src_scale),
              out.data_ptr(), out.numel())
    return out


def _extremum(adj: TiledAdjacency, X: torch.Tensor, reduce: str, return_arg: bool, sub: _Subgraph):
    """(out, arg or None): the element-wise "max" / "min" over the subgraph's neighbours and the winners; one launch."""
    if sub.kw is not None:   # _c_route(0, sub), inline
        res = _call(adj, "_tiled_mm_f32", X, reduce=reduce, return_arg=return_arg, **sub.kw)
        return res[0], res[1] if return_arg else None
    out = torch.empty_like(X)
    arg = torch.empty(X.shape, dtype=torch.int32, device=X.device) if return_arg else None
    _c_launch("extremum", X, "qgtc_tiledmax_f32", 0, adj, sub, X.data_ptr(), X.numel(), X.size(1), 0 if reduce == "max" else 1,
              out.data_ptr(), out.numel(), _ptr(arg), 0 if arg is None else arg.numel())
    return out, arg


def _att(adj: TiledAdjacency, X: torch.Tensor, **kw):
    """The ``att_mode`` keyword overload of the binding on this view (include/qgtc.h, "Attention tiled products")."""
    return _call(adj, "_tiled_mm_f32", X, **kw)


def _att_heads_product(adj: TiledAdjacency, X: torch.Tensor, att_own: torch.Tensor, att_nbr: torch.Tensor, slope: float, backward: bool,
                       shift: torch.Tensor, inv, sub: _Subgraph):
    """The C-entry route of :func:`_att_product` - qgtc_tiledatt_heads_f32 and its twins for scores [n, H], qgtc_tiledatt_f32_fanout and
    its twins for one head over a sample -, one launch on the current stream for all heads. The statistics have the scores' shape."""
    out = torch.empty_like(X)
    m = None if backward else torch.empty(att_own.shape, dtype=torch.float32, device=adj.device)
    if not backward:
        inv = torch.empty_like(m)
    _c_launch("attention product", X, "qgtc_tiledatt_f32", att_own.size(1) if att_own.dim() == 2 else 0, adj, sub, X.data_ptr(), X.numel(),
              X.size(1), att_own.data_ptr(), att_nbr.data_ptr(), slope, int(backward), shift.data_ptr(), None if backward else m.data_ptr(),
              inv.data_ptr(), out.data_ptr(), out.numel())
    return (out,) if backward else (out, m, inv)


def _att_product(adj: TiledAdjacency, X: torch.Tensor, att_own: torch.Tensor, att_nbr: torch.Tensor, slope: float, backward: bool,
                 shift: torch.Tensor, inv, sub: _Subgraph):
    """The softmax-weighted product over the subgraph, one launch. Forward: ``shift`` is M, the largest neighbour score of every row
    (and head), and the result (out, m, inv); backward (on the other view, the scores swapped): ``shift`` and ``inv`` are the forward's
    m and inv and the result (out,)."""
    if _c_route(att_own.dim() == 2, sub):
        return _att_heads_product(adj, X, att_own, att_nbr, slope, backward, shift, inv, sub)
    if backward:
        return _att(adj, X, att_mode="backward", att_own=att_own, att_nbr=att_nbr, negative_slope=slope, shift=shift, inv=inv,
                    **sub.kw)
    return _att(adj, X, att_mode="forward", att_own=att_own, att_nbr=att_nbr, negative_slope=slope, shift=shift, **sub.kw)


def _att_heads_grad(adj: TiledAdjacency, A: torch.Tensor, B: torch.Tensor, att_own: torch.Tensor, att_nbr: torch.Tensor, slope: float,
                    nbr_owns: bool, m: torch.Tensor, inv: torch.Tensor, D: torch.Tensor, sub: _Subgraph) -> torch.Tensor:
    """The C-entry route of :func:`_att_grad`: qgtc_tiledatt_grad_heads_f32 and its twins, qgtc_tiledatt_grad_f32_fanout and its twins;
    one launch on the current stream for all heads. The gradient has the scores' shape."""
    out = torch.empty(att_own.shape, dtype=torch.float32, device=adj.device)
    _c_launch("score gradient", A, "qgtc_tiledatt_grad_f32", att_own.size(1) if att_own.dim() == 2 else 0, adj, sub, A.data_ptr(),
              B.data_ptr(), A.numel(), A.size(1), att_own.data_ptr(), att_nbr.data_ptr(), slope, int(nbr_owns), m.data_ptr(), inv.data_ptr(),
              D.data_ptr(), out.data_ptr(), out.numel())
    return out


def _att_grad(adj: TiledAdjacency, A: torch.Tensor, B: torch.Tensor, att_own: torch.Tensor, att_nbr: torch.Tensor, slope: float,
              nbr_owns: bool, m: torch.Tensor, inv: torch.Tensor, D: torch.Tensor, sub: _Subgraph) -> torch.Tensor:
    """The gradient of a score over the subgraph, one launch: the out node's (``nbr_owns`` False, on the forward's view, A = dY and
    B = X) or the neighbour's (True, on the other view, A = X and B = dY, the scores swapped)."""
    if _c_route(att_own.dim() == 2, sub):
        return _att_heads_grad(adj, A, B, att_own, att_nbr, slope, nbr_owns, m, inv, D, sub)
    return _att(adj, A, att_mode="grad_nbr" if nbr_owns else "grad_own", att_own=att_own, att_nbr=att_nbr, negative_slope=slope, shift=m,
                inv=inv, other=B, D=D, **sub.kw)[0]


def _att_heads_rowdot(A: torch.Tensor, B: torch.Tensor, H: int) -> torch.Tensor:
    """float32 [n, H] of qgtc_rowdot_heads_f32: DOT of every head's columns of A[o] and B[o], one launch on the current stream."""
    out = torch.empty((A.size(0), H), dtype=torch.float32, device=A.device)
    _c_call("the row dot with heads", A, getattr(_c_abi(), _c_name("qgtc_rowdot_f32", H, False)), A.data_ptr(), B.data_ptr(), A.numel(),
            A.size(0), A.size(1), out.data_ptr(), out.numel(), H)
    return out


def _rowdot(adj: TiledAdjacency, A: torch.Tensor, B: torch.Tensor, heads: int) -> torch.Tensor:
    """DOT(A[o], B[o]) of every row, per head with ``heads``: one launch. It walks no tile, so it has no subgraph; the binding takes it
    through the view's ``att_mode`` overload all the same."""
    return _att_heads_rowdot(A, B, heads) if _c_route(heads, _ALL) else _att(adj, A, att_mode="rowdot", other=B)[0]


def _attention(adj: TiledAdjacency, X: torch.Tensor, att_out: torch.Tensor, att_nbr: torch.Tensor, slope: float, sub: _Subgraph):
    """(out, m, inv): the max launch on the neighbours' scores gives M, the largest neighbour score of every row (and head), then one
    product launch. Both run over the subgraph: M must be the maximum over the KEPT neighbours, or the weights' sum could fall below 1."""
    p, q = att_out.detach(), att_nbr.detach()
    if q.dim() == 2:   # a score per head: the same two launches carry all heads (include/qgtc_attn_heads.h)
        M = _extremum(adj, q, "max", False, sub)[0]
    else:
        M = _extremum(adj, q.unsqueeze(1), "max", False, sub)[0].reshape(adj.n)
    return _att_product(adj, X, p, q, slope, False, M, None, sub)


def _scale_name(row_scale) -> str:
    """The scale a refusal names when one is set: ``row_scale`` before ``src_scale``."""
    return "src_scale" if row_scale is None else "row_scale"


def _resolve(adj: TiledAdjacency, X, row_scale, src_scale, reduce, return_arg, attn, negative_slope, return_stats, edge_drop, row_mask,
             nbr_mask, edge_weight, fanout=None):
    """(mode, subgraph, slope) of a call of :func:`tiledMMFloat` / :func:`tiledAggregate`, or the refusal it earns. ``mode`` is
    "weighted" (``edge_weight``), "attention" (``attn``), "extremum" (``reduce`` "max" / "min") or "sum" (plain or scaled); ``subgraph``
    the :class:`_Subgraph` of the checked ``edge_drop``, node masks or ``fanout`` - ``_ALL`` without any, and a pair (k, seed) is drawn
    here, by one selection launch after every refusal -; ``slope`` the checked ``negative_slope`` of the attention. This is the one table
    of what may be combined, in the order the refusals are made: the masks, ``reduce``, then per mode what it does not take and its
    operands. A new variant adds its row here."""
    _check(adj)
    key, slope = _edge_drop_key(edge_drop), None
    masked = row_mask is not None or nbr_mask is not None
    if masked:
        if row_mask is not None:
            _check_mask(adj, row_mask, "row_mask")
        if nbr_mask is not None:
            _check_mask(adj, nbr_mask, "nbr_mask")
        if key is not None:
            raise ValueError("row_mask / nbr_mask cannot be combined with edge_drop: not built")
    if fanout is not None:
        check_fanout(adj, fanout)
        for name, on in (("edge_drop", key is not None), ("row_mask / nbr_mask", masked), ("edge_weight", edge_weight is not None),
                         ("[n, H] scores", isinstance(attn, (tuple, list)) and len(attn) == 2
                          and bool(_attn_heads(adj, attn[0]) or _attn_heads(adj, attn[1])))):
            if on:
                raise ValueError(f"fanout cannot be combined with {name}: not built")
    if reduce not in ("sum", "max", "min"):
        raise ValueError(f'reduce must be "sum", "max" or "min", not {reduce!r}')
    if edge_weight is not None:
        _check_edge_weight(adj, edge_weight, src_scale, key, masked, reduce, attn, X)
        if return_arg or return_stats:
            raise ValueError("return_arg / return_stats cannot be combined with edge_weight: not built")
        mode = "weighted"
    elif attn is not None:
        if row_scale is not None or src_scale is not None:
            raise ValueError(f"{_scale_name(row_scale)} cannot be combined with attn")
        if reduce != "sum":
            raise ValueError(f'attn cannot be combined with reduce="{reduce}"')
        if return_arg:
            raise ValueError("return_arg cannot be combined with attn: a weighted sum has no winning neighbour")
        slope = _check_slope(negative_slope)
        _check_float_operand(adj, X)
        _check_attn(adj, attn, X)
        mode = "attention"
    elif return_stats:
        raise ValueError("return_stats needs attn: only the attention product has softmax statistics")
    elif reduce == "sum":
        if return_arg:
            raise ValueError('return_arg needs reduce="max" or "min": a sum has no winning neighbour')
        mode = "sum"
    else:
        if row_scale is not None or src_scale is not None:
            raise ValueError(f'{_scale_name(row_scale)} cannot be combined with reduce="{reduce}"')
        mode = "extremum"
    if mode != "attention":   # which has checked its operands, and takes no scale
        _check_float_operand(adj, X)
        if row_scale is not None:
            _check_scale(adj, row_scale)
        if src_scale is not None:
            _check_scale(adj, src_scale, "src_scale")
    # after every refusal: the common call constructs nothing, and a pair (k, seed) is drawn here
    if key is None and not masked and fanout is None:
        return mode, _ALL, slope
    return mode, _Subgraph.of(key, row_mask, nbr_mask, None if fanout is None else as_sample(adj, fanout)), slope


def tiledMMFloat(adj: TiledAdjacency, X: torch.Tensor, row_scale: torch.Tensor | None = None,
                 src_scale: torch.Tensor | None = None, reduce: str = "sum", return_arg: bool = False, attn=None,
                 negative_slope: float = 0.2, return_stats: bool = False, edge_drop=None, row_mask: torch.Tensor | None = None,
                 nbr_mask: torch.Tensor | None = None, edge_weight: torch.Tensor | None = None, fanout=None):
    """float32 [n, N] = A . X for a float32 ``X`` [n, N] (contiguous, on the adjacency's device, rows in the adjacency's numbering);
    on ``adj.T``, A^T . X. Every output row adds the rows of X of its neighbours in ASCENDING id order, starting from +0, one float32
    add each; with ``row_scale`` (as in :func:`tiledMM2Int`) the row is then multiplied by row_scale[r], one float32 multiply. The
    result is the same bits on every launch; a NaN or an infinity in X[v] reaches exactly the rows adjacent to v; for integer X with
    sums below 2^24 it equals ``tiledMM2Int`` on the packed planes of X. Nothing is converted or copied: another dtype is a
    TypeError, another shape, device or a non-contiguous X a ValueError. On a reordered adjacency ``to_new`` / ``to_old`` move X and
    the result (the adds then follow the new ids).

    With ``src_scale`` (float32 [n], like ``row_scale``) neighbour v's row is multiplied by src_scale[v] as it is added - one float32
    multiply, then the add, not fused -, so the result is diag(row_scale) . A . diag(src_scale) . X, bit for bit
    ``tiledMMFloat(adj, src_scale[:, None] * X, row_scale)`` without the elementwise pass. Without it the call is the one it was.

    ``reduce="max"`` / ``"min"`` give the element-wise extremum over each row's neighbours instead of their sum (include/qgtc.h,
    "Extremum tiled products"): out[r, c] is the word X[v, c] of the winning neighbour v, bit for bit - the first NaN in id order,
    otherwise the lowest id among those attaining the extremum (-0 and +0 compare equal) -, and +0 for a row without neighbours.
    ``return_arg=True`` returns ``(out, arg)`` with arg int32 [n, N], the winner in the adjacency's numbering, -1 for a row without
    neighbours. A scale with "max" / "min", ``return_arg`` with "sum" and any other ``reduce`` are a ValueError.

    ``attn=(att_out, att_nbr)`` (float32 [n] each, like a scale) gives the softmax-weighted sum of GAT instead (include/qgtc.h,
    "Attention tiled products"): out[o] = sum over o's neighbours k, ascending, of w[o, k] . X[k], divided by the sum of the w, with
    w[o, k] = EXP(L(att_out[o] + att_nbr[k]) - m[o]), L the leaky ReLU of ``negative_slope`` (in [0, 1]) and m[o] the row's largest
    logit; every operation is one float32 operation in a fixed order, EXP included, so the result is the same bits on every launch.
    att_nbr[k] = -inf masks neighbour k (slope > 0; a row needs one unmasked neighbour); a row without neighbours gives +0.
    ``return_stats=True`` returns ``(out, m, inv)`` with inv float32 [n] the reciprocal of the weights' sum (0 without neighbours).
    ``attn`` with a scale, with ``reduce`` other than "sum" or with ``return_arg``, ``return_stats`` without ``attn`` and a slope
    outside [0, 1] are a ValueError. It is a max launch on the scores plus one product launch.

    The scores may also be float32 [n, H] each, contiguous, of one shape, with H >= 2 dividing N: a score per node and HEAD, head h being
    the columns h d .. (h + 1) d - 1 of X and of the result (d = N / H). Column c takes the softmax of head c // d; the operations and
    their order are the same, so every head is bit for bit the 1-D call on its contiguous slice, in the same two launches
    (include/qgtc_attn_heads.h). ``return_stats=True`` then gives m and inv as [n, H]. ``att_nbr[k, h] = -inf`` masks neighbour k in head
    h only. ``edge_drop`` and the node masks below work as for one head. [n, 1] stays the ValueError it was (pass the 1-D vector); two
    scores of different shapes and an H that does not divide N are a ValueError.

    ``edge_drop=(rate, seed)`` (rate a float in [0, 1), seed an int in [0, 2^64)), in every mode above, aggregates over a random subgraph
    (include/qgtc.h, "Edge dropout"): cell (i, j) of the adjacency - row i, column j, on ``adj.T`` still the cell of ``adj`` - is kept when
    the 32-bit hash H(i, j, seed) is at least floor(rate * 2^32), and the result is bit for bit the same call on
    ``pack_edges_tiled`` of the kept edges: the folds run over the kept neighbours in ascending id order, a dropped neighbour's row is
    never loaded, nothing is rescaled, and a row that loses every neighbour is a row without neighbours (+0, arg -1, inv 0). Rate 0
    gives the plain call's bits. The mask is in the ADJACENCY'S OWN numbering: on a reordered adjacency i and j are the new ids, so the
    same seed masks other edges of the original graph than it would without the reordering. The seed is a kernel argument: a captured
    graph replays ONE mask (recapture, or draw the subgraph outside the graph, for a fresh one per step). A rate outside [0, 1) or NaN
    and a seed outside [0, 2^64) are a ValueError, anything but a pair (or a seed that is no int) a TypeError.

    ``row_mask`` / ``nbr_mask`` (int32 bitmaps of :func:`node_bitmap`, each optional, relative to this view like the scales, in the
    adjacency's own numbering), in every mode above, restrict the fold to a subgraph (include/qgtc.h, "Node masks"): row o is computed
    iff o is in ``row_mask`` and holds what a row without neighbours holds otherwise (+0, times row_scale[o]; arg -1; inv 0); neighbour
    k takes part iff k is in ``nbr_mask``, and a neighbour outside it is never
    loaded, so a NaN in its row reaches nothing. The result is bit for bit the same call on ``pack_edges_tiled`` of the edges whose row
    end lies in ``row_mask`` and whose neighbour end lies in ``nbr_mask``; all-ones masks give the plain call's bits. A 32-row block
    (on ``adj.T``: a 128-row k-quad) without a live row reads no tile. The masks are kernel arguments read on the device: a captured
    graph follows the bitmap's contents. Another dtype is a TypeError; another length, device or a non-contiguous mask a ValueError; a
    mask with ``edge_drop`` a ValueError (not built).

    ``edge_weight`` (float32 [nnz] in slot order, from :func:`edge_values`; include/qgtc.h, "Edge values") weighs every edge:
    ``out[i] = row_scale[i] * sum over i's neighbours j of this view, ascending, of fl(values[slot] * X[j])``, the slot being that of
    the cell of ``adj`` whichever the view - one float32 multiply, then the add, not fused. All ones give the plain call's bits;
    ``values = c[col]`` (:func:`edge_endpoints`) gives ``src_scale=c`` on ``adj``. ``row_scale`` stays available. The values are a
    kernel argument read on the device: a captured graph follows their contents. Another dtype is a TypeError; another length or
    device or a non-contiguous vector a ValueError; ``edge_weight`` with ``src_scale``, ``edge_drop``, a node mask, ``reduce`` other than
    "sum" or ``attn`` a ValueError (not built: fold a source scale into the weights with :func:`edge_endpoints`).

    ``edge_weight`` may also be float32 [nnz, H], contiguous, with H dividing N: a weight per stored cell and HEAD, head h being the
    columns h d .. (h + 1) d - 1 of X and of the result (d = N / H). Column c takes ``values[slot, c // d]``; the operations and their
    order are the same, so every head is bit for bit the 1-D call on its contiguous slice, in one launch (include/qgtc_heads.h).
    H is at least 2: [nnz, 1] stays the ValueError it was (pass the 1-D vector). Whatever is refused with a 1-D ``edge_weight`` is
    refused with this one in the same words; an H that does not divide N is a ValueError.

    ``fanout=(k, seed)`` (k an int >= 1, the seed as for ``edge_drop``) aggregates over a fixed-fanout sample instead
    (include/qgtc_fanout.h): at most k neighbours per output row of the view passed, drawn by one selection launch - the k cells of the
    row with the largest hashes H(i, j, seed), exactly min(deg, k) of them, a uniform draw without replacement - and then the result is
    bit for bit the same call on ``pack_edges_tiled`` of the kept edges, as under ``edge_drop``. ``fanout`` may also be a
    ``fanout.FanoutSample`` (``fanout.sample_fanout(view, k, seed)``): on the view it was taken on the thresholds are the output rows', on
    the other view the neighbours' - the same kept cells, which is what a backward needs - and no selection is launched. Built for the sum
    with either scale, ``reduce="max"`` / ``"min"`` with ``return_arg`` and one-head ``attn`` with ``return_stats``; k at least the largest
    degree gives the plain call's bits. A k below 1 is a ValueError, a k that is no int a TypeError; a sample of another adjacency is a
    ValueError; ``fanout`` with ``edge_drop``, a node mask, ``edge_weight`` or [n, H] scores a ValueError (not built)."""
    mode, sub, slope = _resolve(adj, X, row_scale, src_scale, reduce, return_arg, attn, negative_slope, return_stats, edge_drop,
                                row_mask, nbr_mask, edge_weight, fanout)
    if mode == "sum":
        return _sum(adj, X, row_scale, src_scale, sub)
    if mode == "extremum":
        out, arg = _extremum(adj, X, reduce, bool(return_arg), sub)
        return (out, arg) if return_arg else out
    if mode == "attention":
        out, m, inv = _attention(adj, X, attn[0], attn[1], slope, sub)
        return (out, m, inv) if return_stats else out
    return _weighted(adj, X, row_scale, edge_weight)


def _weighted(adj: TiledAdjacency, X: torch.Tensor, row_scale, values: torch.Tensor) -> torch.Tensor:
    """The weighted sum, qgtc_tiledmm_f32_edge_heads / _t_edge_heads through the binding's ``edge_values`` keyword: one launch on the
    current stream. ``values`` [nnz] is one head; [nnz, H] weighs column c by ``values[slot, c // (N / H)]``."""
    val_ptr, val_row, _ = _value_index(adj)
    return _call(adj, "_tiled_mm_f32", X, row_scale, edge_values=(val_ptr, val_row, values))


def _tiled_select(adj: TiledAdjacency, dY: torch.Tensor, arg: torch.Tensor) -> torch.Tensor:
    """float32 [n, N]: row v adds, in ascending id order, dY[r] of its neighbours r where arg[r] names v (include/qgtc.h, "Extremum
    tiled products", the select). On the other view of a max / min forward with that forward's arg it is the gradient for X."""
    return _call(adj, "_tiled_mm_f32", dY, reduce="select", arg=arg)[0]


class _TiledAggregate(torch.autograd.Function):
    """Y = diag(r) . A . diag(c) . X, so dX = diag(c) . A^T . diag(r) . dY: the same product on the other view, scales swapped - and
    node masks swapped: a neighbour of the forward is an output row of the backward. The product is linear in X, so the backward is
    this Function again, on the other view: it can be differentiated in turn, and the second derivative is the forward on the other
    operand. Without a graph to build (``create_graph=False``) that is the one launch it always was."""

    @staticmethod
    def forward(ctx, adj, X, row_scale, src_scale, sub=_ALL):
        ctx.adj, ctx.sub = adj, sub   # a sample was taken once, by _resolve
        ctx.save_for_backward(row_scale, src_scale, *sub.tensors())
        return _sum(adj, X, row_scale, src_scale, sub)

    @staticmethod
    def backward(ctx, dY):
        dX = None
        if ctx.needs_input_grad[1]:
            row_scale, src_scale, *mine = ctx.saved_tensors
            dX = _TiledAggregate.apply(ctx.adj.T, dY.contiguous(), src_scale, row_scale, ctx.sub.rebuilt(mine).other())
        return None, dX, None, None, None


class _TiledWeighted(torch.autograd.Function):
    """Y = diag(r) . (A o W) . X with W the edge values: dX = (A o W)^T . diag(r) . dY, the weighted product on the other view, and
    dW[slot(i, j)] = DOT(r[i] dY[i], X[j]), one SDDMM - each launched only when its gradient is needed. With values [nnz, H] both
    are the entries with heads: still one launch each."""

    @staticmethod
    def forward(ctx, adj, X, row_scale, values):
        ctx.adj = adj
        ctx.save_for_backward(X, values, row_scale)
        return tiledMMFloat(adj, X, row_scale, edge_weight=values)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dY):
        X, values, row_scale = ctx.saved_tensors
        dX = dV = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[3]:
            dY = dY.contiguous()
            if row_scale is not None:
                dY = row_scale[:, None] * dY
            if ctx.needs_input_grad[1]:
                dX = tiledMMFloat(ctx.adj.T, dY, edge_weight=values)
            if ctx.needs_input_grad[3]:
                dV = tiledSDDMM(ctx.adj, dY, X, values.size(1) if values.dim() == 2 else 1)
        return None, dX, None, dV


class _TiledExtremum(torch.autograd.Function):
    """Y[r] = X[arg[r]] element by element, so dX[v] = the sum of dY[r] over the rows r that chose v: the select on the other view."""

    @staticmethod
    def forward(ctx, adj, X, reduce, sub=_ALL):
        out, arg = _extremum(adj, X, reduce, True, sub)
        ctx.adj = adj
        ctx.save_for_backward(arg)   # the select needs no mask: arg names kept (participating) neighbours only
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dY):
        dX = None
        if ctx.needs_input_grad[1]:
            arg, = ctx.saved_tensors
            dX = _tiled_select(ctx.adj.T, dY.contiguous(), arg)
        return None, dX, None, None


class _TiledAttention(torch.autograd.Function):
    """Y[o] = sum_k alpha[o, k] . X[k] with alpha the softmax of L(p[o] + q[k]) over o's neighbours. With D[o] = dY[o] . Y[o]:
    dX[k] = sum_o alpha[o, k] . dY[o] (the product on the other view, weights rebuilt from the neighbour's m and inv), and the logit
    of edge (o, k) gets u = alpha[o, k] . (dY[o] . X[k] - D[o]) . L'(e), which dp folds over k on this view and dq over o on the other."""

    @staticmethod
    def forward(ctx, adj, X, att_out, att_nbr, slope, sub=_ALL):
        out, m, inv = _attention(adj, X, att_out, att_nbr, slope, sub)
        ctx.adj, ctx.slope, ctx.sub = adj, slope, sub   # a sample was taken once, by _resolve: every gradient launch reuses it
        ctx.save_for_backward(X, att_out, att_nbr, out, m, inv, *sub.tensors())
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dY):
        X, p, q, Y, m, inv, *mine = ctx.saved_tensors
        adj, other, slope = ctx.adj, ctx.adj.T, ctx.slope
        need_x, need_p, need_q = ctx.needs_input_grad[1:4]
        dY = dY.contiguous()
        # every gradient walks the forward's subgraph: as it is on this view (dp), as the other view sees it there (dX and dq)
        here = ctx.sub.rebuilt(mine)
        there = here.other()
        dX = dp = dq = None
        if need_x:
            dX = _att_product(other, dY, q, p, slope, True, m, inv, there)[0]
        if need_p or need_q:
            D = _rowdot(adj, dY, Y, p.size(1) if p.dim() == 2 else 0)
            if need_p:
                dp = _att_grad(adj, dY, X, p, q, slope, False, m, inv, D, here)
            if need_q:
                dq = _att_grad(other, X, dY, q, p, slope, True, m, inv, D, there)
        return None, dX, dp, dq, None, None


def tiledAggregate(adj: TiledAdjacency, X: torch.Tensor, row_scale: torch.Tensor | None = None,
                   src_scale: torch.Tensor | None = None, reduce: str = "sum", attn=None, negative_slope: float = 0.2,
                   edge_drop=None, row_mask: torch.Tensor | None = None, nbr_mask: torch.Tensor | None = None,
                   edge_weight: torch.Tensor | None = None, fanout=None) -> torch.Tensor:
    """:func:`tiledMMFloat` under ``torch.autograd``: the forward is ``tiledMMFloat(adj, X, row_scale, src_scale)`` and the gradient
    for X is ``tiledMMFloat(adj.T, dY, row_scale=src_scale, src_scale=row_scale)`` - one launch each way, both specified to the bit.
    The scales get no gradient: one that requires it is a ValueError. It works on ``adj``, ``adj.T`` and reordered adjacencies
    (``to_new`` / ``to_old`` are ``index_select`` and differentiate by themselves).

    The sum (plain, scaled, under ``edge_drop``, node masks or ``fanout``) is linear in X and has a SECOND derivative: its backward is
    this differentiable call on the other view with the scales and masks swapped and the same sample, so under ``create_graph=True`` the
    gradient carries a graph, and with ``dX = grad(Y, X, dY)`` the derivative of ``<dX, R>`` for dY is the forward on the other operand,
    ``tiledMMFloat(adj, R, ...)`` with the forward's own scales, masks, key or sample, bit for bit. Every other mode below raises when
    its backward is differentiated (``once_differentiable``).

    Every tensor passed to a differentiable call - X, the scores, ``edge_weight``, the scales, the node bitmaps, a ``FanoutSample``'s
    ``thr``, masks and ``counts`` - is kept for the backward by reference through ``save_for_backward``: it must not be edited in place
    before the backward has run, and autograd raises ("modified by an inplace operation") if it was, instead of differentiating another
    graph. The adjacency's own tensors and caches are constant by contract and not checked.

    With ``reduce="max"`` / ``"min"`` the forward is ``tiledMMFloat(adj, X, reduce=reduce)``; it keeps the winners, and the backward
    gives each element of dY to the neighbour that won it (under ties, all of it to the one ``arg`` names): one gather on the other
    view, its adds in ascending id order. There is no second derivative: differentiating the backward raises. A scale with them is a
    ValueError.

    With ``attn=(att_out, att_nbr)`` the forward is ``tiledMMFloat(adj, X, attn=attn, negative_slope=negative_slope)`` and the result is
    differentiable in X, att_out and att_nbr: the gradient for X is one product launch on the other view, the two score gradients are
    a row dot and one launch each (att_out's on this view, att_nbr's on the other); a gradient nobody needs is not launched. All of
    them are specified to the bit (include/qgtc.h, "Attention tiled products") and there is no second derivative. ``attn`` with a
    scale or with ``reduce`` other than "sum" is a ValueError. With scores [n, H] (as in :func:`tiledMMFloat`) the gradients of the
    scores are [n, H] and the backward is still at most five launches for all heads: the product on the other view, one row dot and
    one launch per score gradient, each head bit for bit the single-head call's.

    With ``edge_drop=(rate, seed)`` (as in :func:`tiledMMFloat`, every mode) the forward runs on the random subgraph and every backward
    launch gets the same pair on the other view, where the mask is rebuilt from the same cells of the adjacency: the gradients are those
    of the unmasked call on ``pack_edges_tiled`` of the kept edges, bit for bit. The mask is in the adjacency's own numbering (the new
    ids on a reordered adjacency), and a captured graph replays one mask, because the seed is a kernel argument.

    With ``row_mask`` / ``nbr_mask`` (as in :func:`tiledMMFloat`, every mode) the forward runs on the masked graph and the backward is
    the product on the other view with the masks swapped, like the scales: the gradient of the unmasked call on ``pack_edges_tiled`` of
    the edges between the two sets, bit for bit - rows of X outside ``nbr_mask`` get +0 (times src_scale). The extremum's select needs
    no mask (arg names participants only); the attention takes its softmax shift from the masked max launch, passes the masks unchanged
    to att_out's gradient and swapped to the gradient for X and att_nbr's.

    With ``edge_weight=values`` (as in :func:`tiledMMFloat`, the sum only) the result is differentiable in X and in ``values``:
    ``dX = tiledMMFloat(other view, r[:, None] * dY, edge_weight=values)`` and ``dvalues = tiledSDDMM(adj, r[:, None] * dY, X)``, with r
    the ``row_scale`` (the elementwise pre-multiply is a torch operation and happens only when there is one). A gradient nobody needs
    is not launched; both are specified to the bit and there is no second derivative. The combinations :func:`tiledMMFloat` refuses are
    refused here.

    With ``fanout=(k, seed)`` or a ``fanout.FanoutSample`` (as in :func:`tiledMMFloat`: the sum, max / min, one-head ``attn``) the sample
    is taken ONCE, in the forward - one selection launch for a pair, none for a sample - and every backward launch reuses it on the other
    view in the neighbours' form: the gradients are those of the unmasked call on ``pack_edges_tiled`` of the kept edges, bit for bit."""
    mode, sub, slope = _resolve(adj, X, row_scale, src_scale, reduce, False, attn, negative_slope, False, edge_drop, row_mask, nbr_mask,
                                edge_weight, fanout)
    for name, sc in (("row_scale", row_scale), ("src_scale", src_scale)):
        if isinstance(sc, torch.Tensor) and sc.requires_grad:
            wrt = "X and edge_weight" if mode == "weighted" else "X"
            raise ValueError(f"{name} must not require a gradient: tiledAggregate differentiates with respect to {wrt} only")
    if mode == "weighted":
        return _TiledWeighted.apply(adj, X, row_scale, edge_weight)
    if mode == "attention":
        return _TiledAttention.apply(adj, X, attn[0], attn[1], slope, sub)
    if mode == "extremum":
        return _TiledExtremum.apply(adj, X, reduce, sub)
    return _TiledAggregate.apply(adj, X, row_scale, src_scale, sub)


def _edge_softmax(adj: TiledAdjacency, logits: torch.Tensor):
    """(alpha, m, inv) of qgtc_tiled_edge_softmax_heads_f32 / _t, one launch on the current stream: ``logits`` [nnz] is one head with
    statistics [n]; [nnz, H] gives alpha [nnz, H] and statistics [n, H]."""
    nnz, H = logits.size(0), logits.size(1) if logits.dim() == 2 else 1
    alpha = torch.empty_like(logits)
    m = torch.empty((adj.n, H) if logits.dim() == 2 else adj.n, dtype=torch.float32, device=adj.device)
    inv = torch.empty_like(m)
    head, idx = _view_ptrs(adj)
    _c_call("tiledEdgeSoftmax", m, _c_entry("qgtc_tiled_edge_softmax_heads_f32", False, adj), *head, *idx, logits.data_ptr() if nnz else None, alpha.data_ptr() if nnz else None, nnz, m.data_ptr(), inv.data_ptr(), H)
    return alpha, m, inv


def _edge_softmax_grad(adj: TiledAdjacency, alpha: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """out[slot] = alpha . (g - S[owner]) of qgtc_tiled_edge_softmax_grad_heads_f32 / _t, per head for [nnz, H] vectors: one launch on
    the current stream."""
    nnz, H = alpha.size(0), alpha.size(1) if alpha.dim() == 2 else 1
    out = torch.empty_like(alpha)
    if nnz:
        head, idx = _view_ptrs(adj)
        _c_call("the gradient of tiledEdgeSoftmax", alpha, _c_entry("qgtc_tiled_edge_softmax_grad_heads_f32", False, adj), *head, *idx,
                alpha.data_ptr(), g.data_ptr(), out.data_ptr(), nnz, H)
    return out


class _TiledEdgeSoftmax(torch.autograd.Function):
    """alpha = softmax of the logits over each owner's cells: dlogits[k] = alpha[k] . (g[k] - sum over the owner's cells of alpha . g),
    the grad entry on the same view."""

    @staticmethod
    def forward(ctx, adj, logits):
        alpha, m, inv = _edge_softmax(adj, logits)
        ctx.adj = adj
        ctx.save_for_backward(alpha)
        ctx.mark_non_differentiable(m, inv)
        return alpha, m, inv

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _gm, _gi):
        alpha, = ctx.saved_tensors
        dl = None
        if ctx.needs_input_grad[1]:
            dl = _edge_softmax_grad(ctx.adj, alpha, g.contiguous())
        return None, dl


def tiledEdgeSoftmax(adj: TiledAdjacency, logits: torch.Tensor, return_stats: bool = False):
    """float32 [nnz] in slot order: the softmax of a per-edge vector over each node's neighbourhood (include/qgtc.h, "Edge softmax").
    On ``adj`` the softmax runs over each row's out-neighbours, on ``adj.T`` over each node's in-neighbours; the vectors are the same on
    both views. ``alpha[k] = EXP(l_k - m[o]) * inv[o]`` with m the owner's largest logit and inv the reciprocal of the in-order sum of
    the exponentials over the owner's cells in ascending neighbour id: a fixed sequence of float32 operations, so the result is the same
    bits on every launch; one kernel, no atomics. A ``-inf`` logit masks its edge. With ``return_stats`` the result is ``(alpha, m,
    inv)``, float32 [n] each (+0 and 0 for a node without cells). Differentiable in ``logits`` (one launch on the same view, specified
    to the bit too; no second derivative). ``logits`` is float32 [nnz], contiguous, on the adjacency's device: a wrong dtype is a
    TypeError, a wrong shape, device or stride a ValueError.

    ``logits`` may also be float32 [nnz, H], contiguous: H independent softmaxes in one launch (include/qgtc_heads.h), ``alpha`` then
    [nnz, H] and the statistics [n, H], every head bit for bit the 1-D call on ``logits[:, h]`` - a ``-inf`` masks its edge in its head
    only. H is at least 2: [nnz, 1] stays the ValueError it was (pass the 1-D vector)."""
    _check(adj)
    _check_edge_vector(adj, logits, "logits")
    alpha, m, inv = _TiledEdgeSoftmax.apply(adj, logits)
    return (alpha, m, inv) if return_stats else alpha


class _TiledEdgeScores(torch.autograd.Function):
    """s[slot(i, j)] = DOT(A[i], B[j]) on the view: dA = (view o g) . B and dB = (view o g)^T . A, the weighted products with the incoming
    gradient as the weights - each launched only when its gradient is needed."""

    @staticmethod
    def forward(ctx, adj, A, B, heads):
        ctx.adj = adj
        ctx.save_for_backward(A, B)
        return tiledSDDMM(adj, A, B, heads)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        A, B = ctx.saved_tensors
        dA = dB = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            g = g.contiguous()
            if ctx.needs_input_grad[1]:
                dA = tiledMMFloat(ctx.adj, B, edge_weight=g)
            if ctx.needs_input_grad[2]:
                dB = tiledMMFloat(ctx.adj.T, A, edge_weight=g)
        return None, dA, dB, None


def tiledEdgeScores(adj: TiledAdjacency, A: torch.Tensor, B: torch.Tensor, heads: int = 1) -> torch.Tensor:
    """:func:`tiledSDDMM` under ``torch.autograd``: float32 [nnz] in slot order, ``out[slot(i, j)] = DOT(A[i], B[j])`` for the cells
    (i, j) of this view, differentiable in A and B. With g the incoming gradient, ``dA = tiledMMFloat(adj, B, edge_weight=g)`` and
    ``dB = tiledMMFloat(adj.T, A, edge_weight=g)``: one launch each, only when needed, both specified to the bit; no second
    derivative. With ``heads=H`` > 1 the scores are [nnz, H] as in :func:`tiledSDDMM` and g is too: the same two launches, with a
    weight per cell and head."""
    _check(adj)
    _check_float_operand(adj, A)
    heads = _check_heads(heads, A.size(1))
    return _TiledEdgeScores.apply(adj, A, B, heads)


def tiledEdgeAttention(adj: TiledAdjacency, Q: torch.Tensor, K: torch.Tensor, V: torch.Tensor, scale: float | None = None,
                       heads: int = 1) -> torch.Tensor:
    """Dot-product attention over the graph's edges, float32 [n, N]: row i of the view receives
    ``sum over its neighbours j of softmax_j(scale * DOT(Q[i], K[j])) * V[j]`` - the composition
    ``tiledAggregate(adj, V, edge_weight=tiledEdgeSoftmax(adj, tiledEdgeScores(adj, Q, K) * scale))``: an SDDMM, one float32 torch
    multiply per slot, the edge softmax and the weighted sum. ``scale`` defaults to ``1 / sqrt(Q.size(1))``. Differentiable in Q, K and
    V; every launch of the forward and the backward is specified to the bit and none uses atomics. Q and K are float32 [n, d], V is
    float32 [n, N], in the adjacency's numbering; the rows of the view are the receiving nodes (``adj.T``: a node attends over its
    in-neighbours).

    With ``heads=H`` > 1 it is multi-head attention without a loop over the heads: head h is the columns h d .. (h + 1) d - 1 of Q and
    K (d = Q.size(1) / H) and the columns h dv .. of V and of the result (dv = N / H), ``scale`` defaults to ``1 / sqrt(d)``, and the
    same three launches carry all heads with [nnz, H] edge vectors in between (include/qgtc_heads.h); the backward is five launches
    instead of five per head. Output and gradients are bit for bit those of the single-head call on every head's contiguous slices. H
    must divide the widths of Q and of V: otherwise a ValueError."""
    _check(adj)
    _check_float_operand(adj, Q)
    heads = _check_heads(heads, Q.size(1))
    if heads > 1:
        _check_float_operand(adj, V)
        _check_heads(heads, V.size(1))
    scale = 1.0 / math.sqrt(Q.size(1) // heads) if scale is None else float(scale)
    logits = tiledEdgeScores(adj, Q, K, heads) * scale
    return tiledAggregate(adj, V, edge_weight=tiledEdgeSoftmax(adj, logits))


def _addscore(base: TiledAdjacency, A: torch.Tensor, B: torch.Tensor, att: torch.Tensor, slope: float, heads: int) -> torch.Tensor:
    """float32 [nnz, heads] of qgtc_tiled_addscore_heads_f32 on the untransposed adjacency (the caller has swapped the operands of the
    other view): one launch on the current stream."""
    nnz = _value_index(base)[2]
    out = torch.empty((nnz, heads), dtype=torch.float32, device=base.device)
    if nnz:
        head, idx = _view_ptrs(base)
        _c_call("tiledEdgeAdditiveScores", A, _c_abi().qgtc_tiled_addscore_heads_f32, *head, A.data_ptr(), B.data_ptr(), A.numel(), A.size(1),
                att.data_ptr(), att.numel(), slope, *idx, out.data_ptr(), nnz, heads)
    return out


def _addscore_grad(adj: TiledAdjacency, own: torch.Tensor, nbr: torch.Tensor, att: torch.Tensor, slope: float, g: torch.Tensor, heads: int,
                   want_own: bool, want_P: bool):
    """(d_own, P) of qgtc_tiled_addscore_grad_heads_f32 / _t on this view, float32 [n, N] each or None where not wanted: one launch on
    the current stream for both. ``g`` is the scores' gradient, [nnz] or [nnz, heads] in slot order."""
    nnz = g.size(0)
    if not nnz:   # no cell: every fold is its +0
        return torch.zeros_like(own) if want_own else None, torch.zeros_like(own) if want_P else None
    d_own = torch.empty_like(own) if want_own else None
    P = torch.empty_like(own) if want_P else None
    head, idx = _view_ptrs(adj)
    _c_call("the gradient of tiledEdgeAdditiveScores", own, _c_entry("qgtc_tiled_addscore_grad_heads_f32", False, adj), *head, own.data_ptr(),
            nbr.data_ptr(), own.numel(), own.size(1), att.data_ptr(), att.numel(), slope, d_own.data_ptr() if want_own else None,
            P.data_ptr() if want_P else None, own.numel(), *idx, g.data_ptr(), nnz, heads)
    return d_own, P


class _TiledEdgeAdditiveScores(torch.autograd.Function):
    """s[slot(o, k), h] = ADDSCORE(own[o], nbr[k]; att) on the view: d_own and P (whose column sum is datt) are one launch on the view,
    d_nbr the same entry on the other view with the operands swapped - each launched only when a gradient it produces is needed."""

    @staticmethod
    def forward(ctx, adj, own, nbr, att, slope, heads):
        ctx.adj, ctx.slope, ctx.heads = adj, slope, heads
        ctx.save_for_backward(own, nbr, att)
        A, B = (nbr, own) if adj.transposed else (own, nbr)   # fl(x + y) commutes: the row view's kernel serves both views
        out = _addscore(_base(adj), A, B, att, slope, heads)
        return out if heads > 1 else out.view(-1)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        own, nbr, att = ctx.saved_tensors
        d_own = d_nbr = d_att = None
        need_own, need_nbr, need_att = ctx.needs_input_grad[1:4]
        if need_own or need_nbr or need_att:
            g = g.contiguous()
            if need_own or need_att:
                d_own, P = _addscore_grad(ctx.adj, own, nbr, att, ctx.slope, g, ctx.heads, need_own, need_att)
                if need_att:
                    d_att = P.sum(dim=0).view(att.shape)
            if need_nbr:
                d_nbr, _ = _addscore_grad(ctx.adj.T, nbr, own, att, ctx.slope, g, ctx.heads, True, False)
        return None, d_own, d_nbr, d_att, None, None


def _check_additive(adj: TiledAdjacency, own, nbr, att, negative_slope, heads):
    """The checks of the additive score's operands; (slope, heads) as a float and an int."""
    _check(adj)
    _check_float_operand(adj, own)
    heads = _check_heads(heads, own.size(1))
    if not isinstance(nbr, torch.Tensor) or nbr.dtype != torch.float32:
        raise TypeError("nbr must be a float32 torch.Tensor")
    if nbr.shape != own.shape or nbr.device != own.device or not nbr.is_contiguous():
        raise ValueError(f"nbr must be contiguous, on own's device and of own's shape {list(own.shape)}, not {list(nbr.shape)}")
    if not isinstance(att, torch.Tensor) or att.dtype != torch.float32:
        raise TypeError("att must be a float32 torch.Tensor")
    N = own.size(1)
    if tuple(att.shape) not in ((N,), (heads, N // heads)) or att.device != own.device or not att.is_contiguous():
        raise ValueError(f"att must be contiguous, on own's device and of shape [{N}] or [{heads}, {N // heads}], not {list(att.shape)}")
    return _check_slope(negative_slope), heads


def tiledEdgeAdditiveScores(adj: TiledAdjacency, own: torch.Tensor, nbr: torch.Tensor, att: torch.Tensor, negative_slope: float = 0.2,
                            heads: int = 1) -> torch.Tensor:
    """The additive (GATv2) edge score, float32 [nnz] in slot order or [nnz, H] for ``heads=H`` > 1: for every stored cell of this view,
    owner o and neighbour k, and every head h, ``att[h] . leaky_relu(own[o, head h] + nbr[k, head h])`` - ADDSCORE of
    include/qgtc_addscore.h: one float32 add, the leaky relu, one multiply by att and one add per column, 64 strided partial sums and
    the xor butterfly, never fused, so the result is the same bits on every launch; one launch for all heads, every (slot, head) written
    once, no atomics. On ``adj.T`` the cell is the same one of ``adj`` with ``own`` and ``nbr`` swapped. ``own`` and ``nbr`` are float32
    [n, N], contiguous, in the adjacency's numbering; ``att`` is float32 [N] or [H, N / H], contiguous; ``negative_slope`` lies in
    [0, 1]. Differentiable in ``own``, ``nbr`` and ``att`` (no second derivative): ``own``'s gradient and P, whose column sum
    (``torch.sum``) is ``att``'s, are one launch on this view, ``nbr``'s is the same entry on the other view - each launched only when
    needed, both specified to the bit; the derivative of the leaky relu at 0 is the slope. A wrong dtype is a TypeError; a wrong
    shape, device, stride, slope or ``heads`` a ValueError."""
    slope, heads = _check_additive(adj, own, nbr, att, negative_slope, heads)
    return _TiledEdgeAdditiveScores.apply(adj, own, nbr, att, slope, heads)


def tiledEdgeAdditiveAttention(adj: TiledAdjacency, own: torch.Tensor, nbr: torch.Tensor, V: torch.Tensor, att: torch.Tensor,
                               negative_slope: float = 0.2, heads: int = 1) -> torch.Tensor:
    """GATv2 attention over the graph's edges, float32 [n, Nv]: row o of the view receives ``sum over its neighbours k of
    softmax_k(att . leaky_relu(own[o] + nbr[k])) * V[k]`` - the composition ``tiledAggregate(adj, V,
    edge_weight=tiledEdgeSoftmax(adj, tiledEdgeAdditiveScores(adj, own, nbr, att, negative_slope, heads)))``: three launches forward
    and five backward for all heads, every one specified to the bit, none with atomics. Differentiable in ``own``, ``nbr``, ``V`` and
    ``att``. With ``heads=H`` > 1 head h is the columns h d .. (h + 1) d - 1 of ``own`` / ``nbr`` and h dv .. of ``V`` and of the
    result; H must divide both widths. A row without neighbours receives +0."""
    slope, heads = _check_additive(adj, own, nbr, att, negative_slope, heads)
    if heads > 1:
        _check_float_operand(adj, V)
        _check_heads(heads, V.size(1))
    scores = _TiledEdgeAdditiveScores.apply(adj, own, nbr, att, slope, heads)
    return tiledAggregate(adj, V, edge_weight=tiledEdgeSoftmax(adj, scores))


def add_self_loops(src: torch.Tensor, dst: torch.Tensor, n: int) -> tuple[torch.Tensor, torch.Tensor]:
    """(src, dst) with every existing (i, i) edge removed and exactly one appended for each node 0 .. n-1. The packer quantises
    multiplicity 2 to 0, so loops appended to a list that already holds some would erase those; this keeps one of each. Torch
    operations only, on the edges' device; the other edges keep their order."""
    keep = src != dst
    loops = torch.arange(int(n), dtype=src.dtype, device=src.device)
    return torch.cat([src[keep], loops]), torch.cat([dst[keep], loops.to(dst.dtype)])
