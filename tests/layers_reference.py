"""Dense definitions of the float layers of qgtc_ppopp22_amd/conv.py, written from its docstrings and from the two papers (Kipf and
Welling 2017; Velickovic et al. 2018) as plain torch on the CPU: an n x n matrix built from the raw edge list in the edge list's own
numbering, matrix products, a row softmax. No call into the library, no tiled format, no tiledAggregate. float64 is the reference;
the same code in float32 only sizes the tolerance (:func:`tolerances`). Every function returns the output and, for a given dY, the
gradient for X and for every parameter, worked out by hand (tests/test_layers_reference.py holds them against central differences of the forward).
:func:`sage_layer` (sage.SAGEConv, Hamilton et al. 2017) takes its gradients from torch.autograd instead; its samples are those of
tests/tiled_fanout_model.py and tests/tiled_blocks_model.py, NumPy models of the sampling rule that call nothing in the library either.

``WRONG`` names plausible mistakes; ``wrong=`` evaluates the definition with one of them. They are test aids: the CPU test shows
that the inputs of the GPU test tell each mistake from the definition.

``CASES`` are the inputs shared by tests/test_layers_reference.py (CPU) and tests/test_layers_dense_gpu.py (the real layers)."""
import numpy as np
import torch

import tiled_blocks_model
import tiled_drop_model
import tiled_fanout_model
from tiled_model import random_edges

N_NODES = 300                       # 10 row blocks of 32 and 3 k-quads of 128, the last of each partial
F_IN, HIDDEN, CLASSES = 12, 20, 7
GAT_OUT = 7
DROP_RATE, DROP_SEED = 0.5, 0x0123456789ABCDEF
BATCH, BATCH_SEED = 24, 41          # the seed nodes of a mini-batch chain: how many, and the generator that picks them

WRONG = ("transposed",              # A of the other view
         "scores_swapped",          # e[i, j] = a_src . h_i + a_dst . h_j
         "heads_reversed",          # head k reads the column block of head heads - 1 - k
         "heads_summed",            # concat=False adds the heads instead of averaging them
         "multiplicity_kept",       # a doubled edge counts
         "scales_from_one_view",    # sym: the neighbour scale from the row degree too
         "mean_by_other_degree",    # mean: divided by the column degree of the view
         "full_graph_degrees",      # nodes=: the degrees of the whole graph
         "no_keep_scale",           # edge_drop with aggr="sum": no 1 / (1 - rate)
         "mask_in_old_numbering",   # edge_drop under reorder: the edge list's ids are hashed
         "weights_transposed",      # edge_weight of cell (j, i)
         "mean_by_full_degree",     # sage: the sampled mean divided by deg instead of the kept count
         "rows_not_moved",          # sage under reorder: X read, and the result left, in the adjacency's numbering
         "batch_in_old_numbering")  # sage blocks under reorder: the seed flags handed over in the edge list's numbering


# ---- the adjacency ------------------------------------------------------------------------------------------------------------------

def cells(src, dst, n, wrong=None):
    """bool [n, n], element [s, d]: the stored cells of the edge list in its own numbering. An edge given once is stored, given twice
    it is not, given three times or more it is."""
    count = np.zeros((n, n), dtype=np.int64)
    np.add.at(count, (np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)), 1)
    if wrong == "multiplicity_kept":
        return count >= 1
    return (count == 1) | (count >= 3)


def dense_adjacency(src, dst, n, view="adj", wrong=None):
    """bool [n, n]: row i holds the neighbours row i of the view aggregates over - on "adj" the targets of i's edges, on "adj.T" the
    sources of the edges into i."""
    assert view in ("adj", "adj.T")
    a = cells(src, dst, n, wrong)
    return np.ascontiguousarray(a.T if (view == "adj.T") != (wrong == "transposed") else a)


def _oriented(m, view, wrong):
    return m.T if (view == "adj.T") != (wrong == "transposed") else m


def _graph(src, dst, n, view, nodes, edge_drop, wrong):
    """(kept, full): bool [n, n] in the view's orientation - the cells the aggregates run over, and the cells ``norm`` counts (the
    induced subgraph under ``nodes``, the whole graph under ``edge_drop``)."""
    a = cells(src, dst, n, wrong)
    whole = a
    if nodes is not None:
        nodes = np.asarray(nodes, dtype=bool)
        a = a & nodes[:, None] & nodes[None, :]
    full = whole if wrong == "full_graph_degrees" else a
    kept = a
    if edge_drop is not None:
        rate, seed, rank = edge_drop
        ids = np.arange(n, dtype=np.int64) if rank is None or wrong == "mask_in_old_numbering" else np.asarray(rank, dtype=np.int64)
        # cell (s, d) of A, whichever view aggregates: hashed on its ids in the adjacency's numbering
        keep = tiled_drop_model.kept(ids[:, None], ids[None, :], seed, tiled_drop_model.threshold(rate))
        kept = a & keep
    return np.ascontiguousarray(_oriented(kept, view, wrong)), np.ascontiguousarray(_oriented(full, view, wrong))


def _reciprocal(deg, dtype, root):
    d = torch.as_tensor(deg, dtype=dtype)
    s = torch.sqrt(d) if root else d
    return torch.where(d > 0, 1.0 / torch.where(d > 0, s, torch.ones_like(s)), torch.zeros_like(s))


def _scales(full, norm, dtype, wrong):
    """(row, nbr) or None each: the row scale from the row degree of the view, the neighbour scale from the other degree; degree 0
    gives scale 0."""
    row_deg, col_deg = full.sum(axis=1), full.sum(axis=0)
    if norm is None:
        return None, None
    if norm == "mean":
        return _reciprocal(col_deg if wrong == "mean_by_other_degree" else row_deg, dtype, False), None
    assert norm == "sym"
    return _reciprocal(row_deg, dtype, True), _reciprocal(row_deg if wrong == "scales_from_one_view" else col_deg, dtype, True)


class Record:
    """Collects the intermediates of a run: (name, tensor, bound), bound an elementwise bound on every partial sum behind the tensor
    in any order of summation (for a product, |a| . |b|)."""

    def __init__(self):
        self.items = []

    def add(self, name, t, bound=None):
        self.items.append((name, t, t.abs() if bound is None else bound))
        return t

    def mm(self, name, a, b):
        return self.add(name, a @ b, a.abs() @ b.abs())


class _NoRecord:
    def add(self, name, t, bound=None):
        return t

    def mm(self, name, a, b):
        return a @ b


def _scaled(t, s):
    return t if s is None else s[:, None] * t


# ---- GCN ----------------------------------------------------------------------------------------------------------------------------

def _first_extremum(m, t, order, largest):
    """int64 [n, C]: per row i and column c the neighbour j (m[i, j]) with the extremal t[j, c], the first in ``order`` under a tie;
    -1 for a row without neighbours."""
    n = m.shape[0]
    mo, to = m[:, order], t[order]                                                     # neighbours listed in the adjacency's numbering
    fill = float("-inf") if largest else float("inf")
    vals = torch.where(mo[:, :, None], to[None, :, :], torch.full((), fill, dtype=t.dtype))
    best = vals.max(dim=1).values if largest else vals.min(dim=1).values
    place = torch.arange(n)[None, :, None].expand_as(vals)
    first = torch.where((vals == best[:, None, :]) & mo[:, :, None], place, torch.full((), n)).min(dim=1).values
    has = mo.any(dim=1)[:, None].expand_as(first)
    return torch.where(has, order[first.clamp(max=n - 1)], torch.full((), -1))


def gcn_layer(src, dst, n, X, W_in, W_out, dY, view="adj", norm=None, aggr="sum", nodes=None, edge_weight=None, edge_drop=None,
              rank=None, dtype=torch.float64, wrong=None, record=None):
    """Y = Â (Â X W_in) W_out and its gradients, {"Y", "dX", "dW_in", "dW_out"} (and "dEW" [n, n] with ``edge_weight``).

    Â = diag(row) . A . diag(nbr) under ``norm`` (None, "mean", "sym"); with ``aggr`` "max" / "min" Â is the element-wise extremum over
    a row's neighbours instead: a row without neighbours gives 0 and, under a tie, the gradient goes to the tied neighbour with the
    lowest ``rank`` (int [n], the id in the adjacency's numbering; identity when None). ``nodes`` (bool [n]) restricts A to the induced
    subgraph, degrees included. ``edge_weight`` is a dense [n, n] W, element [s, d] the weight of the stored cell (s, d).
    ``edge_drop=(rate, seed, rank)`` keeps cell (s, d) where tiled_drop_model.kept says so on (rank[s], rank[d]); the degrees stay the
    whole graph's, and for aggr="sum" the row scale is multiplied by float32(1 / (1 - rate))."""
    rec = record if record is not None else _NoRecord()
    X, W_in, W_out, dY = (torch.as_tensor(np.asarray(t), dtype=dtype) for t in (X, W_in, W_out, dY))
    kept, full = _graph(src, dst, n, view, nodes, edge_drop, wrong)
    m = torch.from_numpy(kept)

    if aggr in ("max", "min"):
        assert norm is None and edge_weight is None
        order = torch.argsort(torch.arange(n) if rank is None else torch.as_tensor(np.asarray(rank), dtype=torch.int64))

        def forward(t):
            win = _first_extremum(m, t, order, aggr == "max")
            return torch.where(win >= 0, torch.gather(t, 0, win.clamp(min=0)), torch.zeros((), dtype=dtype)), win

        def backward(g, win):
            out = torch.zeros_like(g)
            return out.scatter_add_(0, win.clamp(min=0), torch.where(win >= 0, g, torch.zeros((), dtype=dtype)))

        T1 = rec.mm("X.W_in", X, W_in)
        H, win1 = forward(T1)
        T2 = rec.mm("H.W_out", H, W_out)
        Y, win2 = forward(T2)
        dT2 = rec.add("dT2", backward(dY, win2))
        dW_out = rec.mm("dW_out", H.T, dT2)
        dH = rec.mm("dH", dT2, W_out.T)
        dT1 = rec.add("dT1", backward(dH, win1))
        return {"Y": Y, "dX": rec.mm("dX", dT1, W_in.T), "dW_in": rec.mm("dW_in", X.T, dT1), "dW_out": dW_out}

    assert aggr == "sum"
    row, nbr = _scales(full, norm, dtype, wrong)
    if edge_drop is not None and wrong != "no_keep_scale":
        keep_scale = torch.tensor(1.0 / (1.0 - float(edge_drop[0])), dtype=torch.float64).to(torch.float32).to(dtype)
        row = torch.full((n,), keep_scale.item(), dtype=dtype) if row is None else row * keep_scale
    M = m.to(dtype)
    if edge_weight is not None:
        W = torch.as_tensor(np.asarray(edge_weight), dtype=dtype)
        if wrong == "weights_transposed":
            W = W.T
        M = M * _oriented(W, view, wrong)

    def agg(name, t):
        return rec.add(name, _scaled(rec.mm(name + " sum", M, _scaled(t, nbr)), row))

    def agg_t(name, g):
        return rec.add(name, _scaled(rec.mm(name + " sum", M.T, _scaled(g, row)), nbr))

    T1 = rec.mm("X.W_in", X, W_in)
    H = agg("H", T1)
    T2 = rec.mm("H.W_out", H, W_out)
    Y = agg("Y", T2)
    dT2 = agg_t("dT2", dY)
    dW_out = rec.mm("dW_out", H.T, dT2)
    dH = rec.mm("dH", dT2, W_out.T)
    dT1 = agg_t("dT1", dH)
    out = {"Y": Y, "dX": rec.mm("dX", dT1, W_in.T), "dW_in": rec.mm("dW_in", X.T, dT1), "dW_out": dW_out}
    if edge_weight is not None:
        # both aggregates read the weights: d/dM of M . T2 and of M . T1, on the stored cells, back in the edge list's orientation
        dM = (rec.mm("dEW second", dY, T2.T) + rec.mm("dEW first", dH, T1.T)) * m.to(dtype)
        dM = _oriented(dM, view, wrong)
        out["dEW"] = rec.add("dEW", dM.T if wrong == "weights_transposed" else dM)
    return out


# ---- GAT ----------------------------------------------------------------------------------------------------------------------------

def gat_layer(src, dst, n, X, W, a_dst, a_src, dY, view="adj", heads=1, concat=True, negative_slope=0.2, nodes=None, edge_drop=None,
              dtype=torch.float64, wrong=None, record=None):
    """One graph attention layer and its gradients, {"Y", "dX", "dW", "da_dst", "da_src"}.

    h = X W; per head k, on its block of h's columns, e[i, j] = L(a_dst[k] . h_i + a_src[k] . h_j) on the cells (i, j) of the view,
    alpha = softmax over the neighbours j of row i, out_k[i] = sum_j alpha[i, j] h_j; a row without neighbours gives 0. The heads are
    concatenated or averaged. L is the leaky ReLU, L(e) = e for e > 0 and slope . e otherwise, so at e = 0 exactly its derivative is
    the slope: the convention include/qgtc.h states for the attention gradients, and torch's own. ``nodes`` and ``edge_drop`` as in
    :func:`gcn_layer`; nothing is rescaled."""
    rec = record if record is not None else _NoRecord()
    X, W, a_dst, a_src, dY = (torch.as_tensor(np.asarray(t), dtype=dtype) for t in (X, W, a_dst, a_src, dY))
    C = W.shape[1] // heads
    assert W.shape[1] == heads * C and a_dst.shape == (heads, C) and a_src.shape == (heads, C)
    kept, _ = _graph(src, dst, n, view, nodes, edge_drop, wrong)
    m = torch.from_numpy(kept)
    has = m.any(dim=1)
    slope = torch.tensor(float(negative_slope), dtype=torch.float32).to(dtype)     # the layer hands the kernels a float32
    h = rec.mm("h", X, W)
    dh = torch.zeros_like(h)
    da_dst, da_src = torch.zeros_like(a_dst), torch.zeros_like(a_src)
    share = 1.0 if concat or wrong == "heads_summed" else 1.0 / heads
    outs = []
    for k in range(heads):
        block = heads - 1 - k if wrong == "heads_reversed" else k
        cols = slice(block * C, (block + 1) * C)
        hk = h[:, cols]
        u, v = (a_src[k], a_dst[k]) if wrong == "scores_swapped" else (a_dst[k], a_src[k])
        p, q = rec.mm(f"p{k}", hk, u[:, None])[:, 0], rec.mm(f"q{k}", hk, v[:, None])[:, 0]
        e = p[:, None] + q[None, :]
        logit = torch.where(e > 0, e, slope * e)
        top = torch.where(has, logit.masked_fill(~m, float("-inf")).max(dim=1).values, torch.zeros((), dtype=dtype))
        w = torch.where(m, torch.exp(logit - top[:, None]), torch.zeros((), dtype=dtype))
        den = w.sum(dim=1)
        alpha = rec.add(f"alpha{k}", w / torch.where(has, den, torch.ones_like(den))[:, None])
        outs.append(rec.mm(f"out{k}", alpha, hk))
        # backward
        g = (dY[:, k * C:(k + 1) * C] if concat else dY) * share
        dalpha = rec.mm(f"dalpha{k}", g, hk.T)
        D = rec.add(f"D{k}", (alpha * dalpha).sum(dim=1), (alpha * dalpha).abs().sum(dim=1))
        dlogit = rec.add(f"dlogit{k}", alpha * (dalpha - D[:, None]))
        de = rec.add(f"de{k}", dlogit * torch.where(e > 0, torch.ones((), dtype=dtype), slope))
        dp = rec.add(f"dp{k}", de.sum(dim=1), de.abs().sum(dim=1))
        dq = rec.add(f"dq{k}", de.sum(dim=0), de.abs().sum(dim=0))
        du, dv = rec.mm(f"du{k}", hk.T, dp[:, None])[:, 0], rec.mm(f"dv{k}", hk.T, dq[:, None])[:, 0]
        if wrong == "scores_swapped":
            da_src[k], da_dst[k] = du, dv
        else:
            da_dst[k], da_src[k] = du, dv
        dh[:, cols] += rec.mm(f"dh{k} values", alpha.T, g) + dp[:, None] * u[None, :] + dq[:, None] * v[None, :]
    Y = torch.cat(outs, dim=1) if concat else rec.add("Y", torch.stack(outs).sum(dim=0) * share)
    return {"Y": Y, "dX": rec.mm("dX", dh, W.T), "dW": rec.mm("dW", X.T, dh), "da_dst": da_dst, "da_src": da_src}


# ---- GraphSAGE ----------------------------------------------------------------------------------------------------------------------

def batch_flags(n=N_NODES):
    """bool [n]: the BATCH seed nodes of the chained cases, in the edge list's numbering."""
    flags = np.zeros(n, dtype=bool)
    flags[np.random.default_rng(BATCH_SEED).permutation(n)[:BATCH]] = True
    return flags


def sage_graph(src, dst, n, view, layers, fanout=None, batch=None, seed=DROP_SEED, rank=None, wrong=None):
    """(kept, full, order): per layer the bool [n, n] matrix whose row i holds the neighbours node i aggregates over, the matrix of all
    the view's cells, and the order in which a maximum lists tied neighbours - all three in the edge list's numbering.

    ``fanout`` None: every layer sees the whole neighbourhood. An int k: tiled_fanout_model.kept_edges of fanout k under ``seed`` on the
    view's axis. A tuple with ``batch`` (bool [n], the seed nodes): the chain of tiled_blocks_model.blocks, input layer first. A sample is
    taken on the ids of the adjacency's numbering, (rank[s], rank[d]) for every cell, from the moved seed flags, and mapped back."""
    a = cells(src, dst, n, wrong)
    flip = (view == "adj.T") != (wrong == "transposed")
    axis = "col" if flip else "row"
    own = np.arange(n, dtype=np.int64)
    new = own if rank is None else np.asarray(rank, dtype=np.int64)
    if wrong in ("rows_not_moved", "batch_in_old_numbering"):
        assert rank is not None, wrong
    ids = own if wrong == "mask_in_old_numbering" else new
    s, d = np.nonzero(a)
    es, ed = ids[s], ids[d]                                    # every cell once, in the numbering the sample is taken in
    if fanout is None:
        assert batch is None
        kept = [(es, ed)] * layers
    elif batch is None:
        assert layers == 1
        kept = [tiled_fanout_model.kept_edges(es, ed, n, int(fanout), seed, axis)]
    else:
        assert len(fanout) == layers
        moved = np.zeros(n, dtype=bool)
        moved[ids] = np.asarray(batch, dtype=bool)             # flags[perm], what to_new gives
        if wrong == "batch_in_old_numbering":
            moved = np.asarray(batch, dtype=bool)
        chain = tiled_blocks_model.blocks(es, ed, n, axis, moved, tuple(fanout), seed)
        kept = [tiled_blocks_model.kept_edges(es, ed, n, b["k"], b["seed"], axis, b["rows"]) for b in chain]
    back = own if wrong == "rows_not_moved" else ids           # not moved: the matrices stay in the adjacency's numbering

    def matrix(ks, kd):
        m = np.zeros((n, n), dtype=bool)
        m[ks, kd] = True
        m = m[back][:, back]
        return np.ascontiguousarray(m.T if flip else m)

    order = torch.arange(n) if wrong == "rows_not_moved" else torch.argsort(torch.from_numpy(new))
    return [matrix(ks, kd) for ks, kd in kept], matrix(es, ed), order


def sage_layer(src, dst, n, X, params, dY, view="adj", aggr="mean", fanout=None, batch=None, seed=DROP_SEED, rank=None,
               dtype=torch.float64, wrong=None, record=None):
    """``len(params)`` SAGEConv layers in a row and their gradients by torch.autograd. ``params`` is a list of (W_self [out, in], b [out],
    W_nbr [out, in]); one layer is Y = X . W_self^T + b + agg(X) . W_nbr^T with agg the mean or (``aggr="max"``) the element-wise maximum
    over the neighbours of :func:`sage_graph`, +0 for a node without any. The mean divides by the number of neighbours that matrix keeps:
    deg, min(deg, k) under a fanout, the masked sample's own count in a block. Under a tie the maximum's gradient goes to the tied
    neighbour with the lowest ``rank`` (the id in the adjacency's numbering; identity when None).

    One layer (``batch`` None) returns {"Y", "dX", "dW_self", "db", "dW_nbr"} for the loss <Y, dY>. A chain (``fanout`` a tuple,
    ``batch`` the seed flags) returns "Y" on the batch rows only, [batch.sum(), out], and the parameter gradients with the layer's index
    appended, for the loss (h . dY)[batch].sum(). With ``record`` the backward is also walked by hand, so that every intermediate of
    it is recorded with its bound; the entries named like a result hold what autograd must give."""
    assert aggr in ("mean", "max")

    def note(name, t, bound=None):          # the forward carries autograd's graph: the record gets detached values
        if record is not None:
            record.add(name, t.detach(), None if bound is None else bound.detach())
        return t

    def mm(name, a, b):
        return note(name, a @ b, a.abs() @ b.abs() if record is not None else None)

    L = len(params)
    kept, full, order = sage_graph(src, dst, n, view, L, fanout, batch, seed, rank, wrong)
    zero = torch.zeros((), dtype=dtype)
    x = torch.as_tensor(np.asarray(X), dtype=dtype).clone().requires_grad_(True)
    dY = torch.as_tensor(np.asarray(dY), dtype=dtype)
    ps = [tuple(torch.as_tensor(np.asarray(p), dtype=dtype).clone().requires_grad_(True) for p in layer) for layer in params]
    rows = None if batch is None else torch.from_numpy(np.asarray(batch, dtype=bool))
    divisor = full.sum(axis=1) if wrong == "mean_by_full_degree" else None
    if wrong == "mean_by_full_degree":
        assert aggr == "mean" and fanout is not None

    h, steps = x, []
    for l, (Ws, b, Wn) in enumerate(ps):
        m = torch.from_numpy(kept[l])
        if aggr == "max":
            win = _first_extremum(m, h.detach(), order, True)
            agg = torch.where(win >= 0, torch.gather(h, 0, win.clamp(min=0)), zero)
            steps.append((h, agg, win))
        else:
            s = _reciprocal(kept[l].sum(axis=1) if divisor is None else divisor, dtype, False)
            M = m.to(dtype)
            agg = note(f"agg{l}", _scaled(mm(f"agg{l} sum", M, h), s))
            steps.append((h, agg, (M, s)))
        own, nbr = mm(f"self{l}", h, Ws.T), mm(f"nbr{l}", agg, Wn.T)
        h = note(f"h{l}", own + b + nbr, h.abs() @ Ws.abs().T + b.abs() + agg.abs() @ Wn.abs().T if record is not None else None)
    if rows is None:
        Y, dH = h, dY
        Y.backward(dY)
    else:
        Y, dH = h[rows], torch.where(rows[:, None], dY, zero)
        (h * dY)[rows].sum().backward()
    tag = (lambda l: "") if rows is None else str
    out = {"Y": Y.detach(), "dX": x.grad}
    for l, (Ws, b, Wn) in enumerate(ps):
        out.update({f"dW_self{tag(l)}": Ws.grad, f"db{tag(l)}": b.grad, f"dW_nbr{tag(l)}": Wn.grad})
    if record is not None:
        with torch.no_grad():
            for l in range(L - 1, -1, -1):
                (Ws, b, Wn), (hin, agg, how) = ps[l], steps[l]
                record.mm(f"dW_self{tag(l)}", dH.T, hin)
                record.add(f"db{tag(l)}", dH.sum(dim=0), dH.abs().sum(dim=0))
                record.mm(f"dW_nbr{tag(l)}", dH.T, agg)
                dagg = record.mm(f"dagg{l}", dH, Wn)
                if aggr == "max":
                    through = torch.zeros_like(hin).scatter_add_(0, how.clamp(min=0), torch.where(how >= 0, dagg, zero))
                    through = record.add(f"dagg{l} scattered", through, torch.zeros_like(hin).scatter_add_(
                        0, how.clamp(min=0), torch.where(how >= 0, dagg.abs(), zero)))
                else:
                    through = record.mm(f"dagg{l} spread", how[0].T, record.add(f"dagg{l} scaled", _scaled(dagg, how[1])))
                direct = record.mm(f"dh{l} self", dH, Ws)
                dH = record.add("dX" if l == 0 else f"dh{l}", direct + through, direct.abs() + through.abs())
    return out


# ---- graphs -------------------------------------------------------------------------------------------------------------------------

def dyadic_graph(seed):
    """(src, dst, nodes) on N_NODES nodes: every in-degree and out-degree lies in {0, 1, 4, 16}, so 1 / deg and 1 / sqrt(deg) are
    powers of two. A disjoint union of a complete digraph with loops on 16 nodes, a fan of 16 sources onto 4 targets (in-degree !=
    out-degree), a 64-node circulant with 4 offsets, a 128-node circulant with 16 offsets, 40 loop-only nodes and 31 isolated nodes;
    50 of the edges are given three times (they stay), 40 absent pairs twice (they vanish); the ids are shuffled. The 4 targets of the
    fan all point at one sink (in-degree 4): a fan that ends at its targets is a dead end for a layer PAIR - the targets' rows are
    empty, so whatever scale the sources' rows get multiplies 0 - and a scale taken from the wrong view would not show in any tensor.
    ``nodes`` (bool) is a subset whose induced degrees stay in the set: the 64-circulant, 20 loop nodes and 16 isolated nodes whole,
    4 nodes of the complete digraph, and 4 sources with all 4 targets of the fan and the sink."""
    rng = np.random.default_rng(seed)
    n = N_NODES
    comp = np.arange(0, 16)
    fan_s, fan_t = np.arange(16, 32), np.arange(32, 36)
    c64, c128 = np.arange(36, 100), np.arange(100, 228)
    loops, sink, isolated = np.arange(228, 268), np.arange(268, 269), np.arange(269, 300)
    s, d = [], []
    s.append(np.repeat(comp, 16)), d.append(np.tile(comp, 16))
    s.append(np.repeat(fan_s, 4)), d.append(np.tile(fan_t, 16))
    s.append(fan_t), d.append(np.repeat(sink, 4))
    for ring, offsets in ((c64, (1, 2, 5, 17)), (c128, (1, 2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47))):
        for o in offsets:
            s.append(ring), d.append(ring[(np.arange(ring.size) + o) % ring.size])
    s.append(loops), d.append(loops)
    s, d = np.concatenate(s), np.concatenate(d)
    present = set(zip(s.tolist(), d.tolist()))
    triple = rng.choice(s.size, size=50, replace=False)
    nodes = np.zeros(n, dtype=bool)
    for part in (c64, loops[:20], isolated[:16], comp[:4], fan_s[:4], fan_t, sink):
        nodes[part] = True
    inside = np.flatnonzero(nodes)
    pairs = []
    while len(pairs) < 40:      # the first 20 inside ``nodes``, so that they matter to the induced subgraph too
        pool = inside if len(pairs) < 20 else np.arange(n)
        a, b = (int(v) for v in rng.choice(pool, size=2))
        if (a, b) not in present and (a, b) not in pairs:
            pairs.append((a, b))
    ps, pd = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    s = np.concatenate([s, s[triple], s[triple], ps, ps])
    d = np.concatenate([d, d[triple], d[triple], pd, pd])
    relabel = rng.permutation(n)
    mix = rng.permutation(s.size)
    shuffled = np.zeros(n, dtype=bool)
    shuffled[relabel[inside]] = True
    return relabel[s][mix].astype(np.int64), relabel[d][mix].astype(np.int64), shuffled


def random_graph(seed):
    """(src, dst, nodes): tiled_model.random_edges with about 6 edges a node - directed, asymmetric, doubled edges present - and a
    random half of the nodes."""
    rng = np.random.default_rng(seed)
    src, dst = random_edges(rng, N_NODES, 6 * N_NODES)
    return src, dst, rng.random(N_NODES) < 0.5


# ---- cases --------------------------------------------------------------------------------------------------------------------------

class Case:
    """One layer configuration with its inputs. ``exact``: the dyadic graph with integer data (bit for bit), else the random graph
    with standard-normal data (within :func:`tolerances`). ``denominator``: the largest power-of-two denominator an intermediate of an
    exact case can have. ``wrong``: the variants that apply."""

    def __init__(self, name, kind, exact, wrong, denominator=None, **options):
        self.name, self.kind, self.exact, self.wrong, self.denominator, self.options = name, kind, exact, tuple(wrong), denominator, options
        for w in self.wrong:
            assert w in WRONG, w

    def __repr__(self):
        return self.name

    @property
    def uses_rank(self):
        """The reference depends on the adjacency's numbering: the drop mask and the fanout sample live in it, and ties of max / min
        go by it."""
        if self.kind == "sage":
            return self.options.get("fanout") is not None or self.options["aggr"] == "max"
        return self.options.get("drop", False) or self.options.get("aggr", "sum") != "sum"

    @property
    def chained(self):
        """A sage case of two layers over the blocks of a mini-batch: ``fanout`` holds one k per layer."""
        return self.kind == "sage" and isinstance(self.options.get("fanout"), tuple)

    def graph(self):
        return GRAPHS["dyadic" if self.exact else "random"]

    def inputs(self):
        """dict of float64 arrays, the same on every call: X, dY and the parameters (and EW, the dense edge weights)."""
        rng = np.random.default_rng([17, [c.name for c in CASES].index(self.name)])
        n, o = N_NODES, self.options
        src, dst, _ = self.graph()

        def draw(*shape):
            return rng.integers(-3, 4, size=shape).astype(np.float64) if self.exact else rng.standard_normal(shape)

        def weight(*shape):
            return rng.integers(-2, 3, size=shape).astype(np.float64) if self.exact else rng.standard_normal(shape)

        if self.kind == "gcn":
            t = {"X": draw(n, F_IN), "W_in": weight(F_IN, HIDDEN), "W_out": weight(HIDDEN, CLASSES), "dY": draw(n, CLASSES)}
            if o.get("edge_weight"):
                t["EW"] = weight(n, n) * cells(src, dst, n)
            return t
        if self.kind == "sage":
            dims = (F_IN, HIDDEN, CLASSES) if self.chained else (F_IN, HIDDEN)
            t = {"X": draw(n, dims[0]), "dY": draw(n, dims[-1])}
            for l, (fi, fo) in enumerate(zip(dims, dims[1:])):
                for name, shape in (("W_self", (fo, fi)), ("b", (fo,)), ("W_nbr", (fo, fi))):   # scaled as torch.nn.Linear scales them
                    t[f"{name}{l}"] = weight(*shape) if self.exact else rng.uniform(-1.0, 1.0, size=shape) / fi ** 0.5
            return t
        heads, width = o["heads"], o["heads"] * GAT_OUT
        t = {"X": draw(n, F_IN), "W": weight(F_IN, width), "dY": draw(n, width if o["concat"] else GAT_OUT)}
        if self.exact:
            t["a_dst"], t["a_src"] = np.zeros((heads, GAT_OUT)), np.zeros((heads, GAT_OUT))
        else:   # scaled as the constructor scales them
            t["W"] = t["W"] / F_IN ** 0.5
            t["a_dst"], t["a_src"] = rng.standard_normal((heads, GAT_OUT)) / GAT_OUT ** 0.5, rng.standard_normal((heads, GAT_OUT)) / GAT_OUT ** 0.5
        return t

    def sage_params(self, t):
        """[(W_self, b, W_nbr)] of the layers of a sage case, from its inputs ``t``."""
        return [(t[f"W_self{l}"], t[f"b{l}"], t[f"W_nbr{l}"]) for l in range(2 if self.chained else 1)]

    def reference(self, view, dtype=torch.float64, rank=None, wrong=None, record=None):
        """The dense definition on this case: dict of tensors, "Y" and the gradients."""
        src, dst, nodes = self.graph()
        t, o = self.inputs(), self.options
        if self.kind == "sage":
            return sage_layer(src, dst, N_NODES, t["X"], self.sage_params(t), t["dY"], view=view, aggr=o["aggr"], fanout=o.get("fanout"),
                              batch=batch_flags() if self.chained else None, seed=DROP_SEED, rank=rank, dtype=dtype, wrong=wrong,
                              record=record)
        common = dict(view=view, nodes=nodes if o.get("nodes") else None, dtype=dtype, wrong=wrong, record=record,
                      edge_drop=(DROP_RATE, DROP_SEED, rank) if o.get("drop") else None)
        if self.kind == "gcn":
            return gcn_layer(src, dst, N_NODES, t["X"], t["W_in"], t["W_out"], t["dY"], norm=o.get("norm"), aggr=o.get("aggr", "sum"),
                             edge_weight=t.get("EW"), rank=rank, **common)
        return gat_layer(src, dst, N_NODES, t["X"], t["W"], t["a_dst"], t["a_src"], t["dY"], heads=o["heads"], concat=o["concat"],
                         negative_slope=o["slope"], **common)


GRAPHS = {"dyadic": dyadic_graph(2024), "random": random_graph(2025)}
_BASE = ("transposed", "multiplicity_kept")
_DROP = ("mask_in_old_numbering",)


def _cases():
    out = []
    for norm, d, extra in ((None, 1, ()), ("mean", 256, ("mean_by_other_degree",)), ("sym", 256, ("scales_from_one_view",))):
        out.append(Case(f"gcn-{norm}", "gcn", True, _BASE + extra, d, norm=norm))
        out.append(Case(f"gcn-{norm}-nodes", "gcn", True, _BASE + extra + (("full_graph_degrees",) if norm else ()), d, norm=norm, nodes=True))
    out.append(Case("gcn-edge_weight", "gcn", True, _BASE + ("weights_transposed",), 1, edge_weight=True))
    out.append(Case("gcn-None-drop", "gcn", True, _BASE + _DROP + ("no_keep_scale",), 1, drop=True))
    out.append(Case("gcn-sym-drop", "gcn", True, _BASE + _DROP + ("no_keep_scale", "scales_from_one_view"), 256, norm="sym", drop=True))
    out.append(Case("gcn-max", "gcn", True, _BASE, 1, aggr="max"))
    out.append(Case("gcn-min", "gcn", True, _BASE, 1, aggr="min"))
    out.append(Case("gcn-max-drop", "gcn", True, _BASE + _DROP, 1, aggr="max", drop=True))
    for heads in (1, 2, 4):
        for concat in (True, False):
            # slope 1/2: alpha is 1 / deg, D carries a second 1 / deg, the average a 1 / heads
            extra = (("heads_reversed",) if heads > 1 and concat else ()) + (("heads_summed",) if heads > 1 and not concat else ())
            out.append(Case(f"gat-zero-h{heads}-{'concat' if concat else 'mean'}", "gat", True, _BASE + extra,
                            512 * (1 if concat else heads), heads=heads, concat=concat, slope=0.5))
    many = ("scores_swapped", "heads_reversed")
    out.append(Case("gat-h1-concat", "gat", False, _BASE + ("scores_swapped",), heads=1, concat=True, slope=0.1))
    out.append(Case("gat-h1-mean", "gat", False, _BASE + ("scores_swapped",), heads=1, concat=False, slope=0.2))
    out.append(Case("gat-h3-concat", "gat", False, _BASE + many, heads=3, concat=True, slope=0.2))
    out.append(Case("gat-h3-mean", "gat", False, _BASE + many + ("heads_summed",), heads=3, concat=False, slope=0.1))
    out.append(Case("gat-h3-nodes", "gat", False, _BASE + many, heads=3, concat=True, slope=0.1, nodes=True))
    out.append(Case("gat-h3-drop", "gat", False, _BASE + many + _DROP, heads=3, concat=True, slope=0.2, drop=True))
    out.append(Case("gcn-sym-random", "gcn", False, _BASE + ("scales_from_one_view",), norm="sym"))
    out.append(Case("gcn-mean-random", "gcn", False, _BASE + ("mean_by_other_degree",), norm="mean"))
    return out


def _sage_cases():
    """The cases of kind "sage", after every other so that no earlier case's inputs move. Exact: fanouts 4 and (4, 2) keep 0, 1, 2 or 4
    of a node's 0, 1, 4 or 16 neighbours, so every mean divides by a power of two - 1/16 over a whole neighbourhood, 1/4 under k = 4,
    1/4 . 1/2 through the chain."""
    moved, sampled, mean = ("rows_not_moved",), _DROP + ("rows_not_moved",), ("mean_by_full_degree",)
    chain = ("batch_in_old_numbering",)
    return [Case("sage-mean", "sage", True, _BASE, 16, aggr="mean"),
            Case("sage-max", "sage", True, _BASE + moved, 1, aggr="max", eval=True),
            Case("sage-mean-fanout", "sage", True, _BASE + sampled + mean, 4, aggr="mean", fanout=4),
            Case("sage-max-fanout", "sage", True, _BASE + sampled, 1, aggr="max", fanout=4),
            Case("sage-mean-blocks", "sage", True, _BASE + sampled + mean + chain, 8, aggr="mean", fanout=(4, 2)),
            Case("sage-max-blocks", "sage", True, _BASE + sampled + chain, 1, aggr="max", fanout=(4, 2)),
            Case("sage-mean-random", "sage", False, _BASE, aggr="mean"),
            Case("sage-mean-fanout-random", "sage", False, _BASE + sampled + mean, aggr="mean", fanout=3),
            Case("sage-mean-blocks-random", "sage", False, _BASE + sampled + mean + chain, aggr="mean", fanout=(3, 2)),
            Case("sage-max-blocks-random", "sage", False, _BASE + sampled + chain, aggr="max", fanout=(3, 2))]


CASES = []
CASES.extend(_cases())
CASES.extend(_sage_cases())
EXACT_CASES = [c for c in CASES if c.exact]
TOLERANCE_CASES = [c for c in CASES if not c.exact]
VIEWS = ("adj", "adj.T")


def tolerances(ref64, ref32):
    """{name: tol}: tol(T) = 8 . max(max|T_f32 - T_f64|, 2^-24 . max|T_f64|), from the reference alone."""
    return {k: 8.0 * max(float((ref32[k].to(torch.float64) - ref64[k]).abs().max()), 2.0 ** -24 * float(ref64[k].abs().max()))
            for k in ref64}
