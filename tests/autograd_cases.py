"""The table of differentiable calls of the autograd tests (tests/test_autograd_contract.py on the CPU, tests/test_autograd_contract_gpu.py
on the device): every ``torch.autograd.Function`` of qgtc_ppopp22_amd, through the public call that crosses it.

A CASE carries a name, the Function classes its graph holds (``functions``), its differentiable LEAVES, its SIDE tensors - every other
tensor the call takes or its backward reads, named by the keyword of ``tiledAggregate`` it travels in (``fanout.thr`` is the ``thr`` of
the sample passed as ``fanout=``) -, what its bits are specified against (``spec``), what a second derivative must do (``second``) and a
builder. The adjacency's own tensors and caches are no side tensors: an adjacency is constant by contract.

``build(env)`` gives a :class:`Live` object on the view of ``env``: fresh device tensors with seeded contents and ``run(tensors)``, the
call on them. Every case runs on ``adj`` and on ``adj.T``. The operator rows use one random graph of ``N_OPS`` = 333 nodes (11 row blocks,
3 k-quads, both ragged; the hub row of tests/tiled_model.py has more than 128 neighbours, so the kernels' queues overflow) with 70
columns (ragged past 64 lanes) and 2 heads; the layer rows use the random graph, sizes and parameters of tests/layers_reference.py.

``second``:  "value"  the call is linear in X: d<dX, R>/d(dY) is ``tiledMMFloat`` on R with the forward's own scales, masks, key or
                      sample, bit for bit (``Live.second``);
             "dense"  a layer that is linear in X: the same derivative against the dense float64 definition (``Live.dense``), within
                      layers_reference.tolerances;
             "raises" the backward is ``once_differentiable``: differentiating it raises;
             "inference" the backward itself raises (no property test runs it).

Importing this module needs neither a GPU nor the built extension (test_autograd_contract.py reads CASES on the CPU)."""
import zlib

import numpy as np

import layers_reference as R
import tiled_blocks_model as bm
from tiled_model import random_edges, set_cells

N_OPS, WIDTH, HEADS = 333, 70, 2
FANOUT_K, SEED = 3, 0x0123456789ABCDEF
BATCH = 40                                   # seed nodes of the mini-batch block
SECONDS = ("value", "dense", "raises", "inference")
VIEWS = ("adj", "adj.T")

# the parameters of tiledAggregate that cannot hold a tensor, and why; every other one must be a leaf or a side tensor of some case
NOT_TENSORS = {"adj": "the adjacency: constant by contract", "reduce": "a string", "negative_slope": "a float",
               "edge_drop": "a pair of numbers (rate, seed)"}


class Case:
    def __init__(self, name, functions, leaves, sides, second, spec, build):
        assert second in SECONDS and leaves and functions
        self.name, self.functions, self.leaves, self.sides = name, tuple(functions), tuple(leaves), tuple(sides)
        self.second, self.spec, self.build = second, spec, build

    def __repr__(self):
        return self.name

    @property
    def keywords(self):
        """The keywords of tiledAggregate this case passes a tensor in: "attn[0]" and "fanout.thr" travel in ``attn`` and ``fanout``."""
        return {n.split(".")[0].split("[")[0] for n in self.leaves + self.sides}


CASES = []


def case(name, functions, leaves, sides, second, spec, build):
    CASES.append(Case(name, functions, leaves, sides, second, spec, build))


class Live:
    """``leaves`` {name: float32 device tensor or module parameter}, ``sides`` {name: device tensor}, ``run(tensors)`` the call on
    ``tensors`` (what :meth:`tensors` gives) and the sides; ``second(R)`` / ``dense(R, dtype)`` as the module docstring says;
    ``drawn(tensors)`` the call that draws its edge seed from torch's CPU generator, where there is one. ``run`` reads the side
    tensors when it is called, so an in-place edit of one reaches the next call."""

    def __init__(self, torch, leaves, run, sides=None, second=None, dense=None, drawn=None):
        self.torch, self.leaves, self.run, self.sides = torch, leaves, run, sides or {}
        self.second, self.dense, self.drawn = second, dense, drawn

    def tensors(self, requires):
        """{name: leaf}: a fresh clone of every plain leaf, requiring a gradient iff named in ``requires``; a module parameter is the
        parameter itself with ``requires_grad`` set accordingly and its ``.grad`` cleared."""
        out = {}
        for name, base in self.leaves.items():
            if isinstance(base, self.torch.nn.Parameter):
                base.requires_grad_(name in requires)
                base.grad = None
                out[name] = base
            else:
                out[name] = base.detach().clone().requires_grad_(name in requires)
        return out


# ---- environments -------------------------------------------------------------------------------------------------------------------

def ops_graph():
    """(src, dst) of the operator rows, with the hub row asserted"""
    src, dst = random_edges(np.random.default_rng(1), N_OPS, 6 * N_OPS + 5)
    cells = set_cells(src, dst, N_OPS)
    assert np.bincount(cells // N_OPS, minlength=N_OPS).max() >= 128 and np.bincount(cells % N_OPS, minlength=N_OPS).max() >= 128
    return src, dst


GRAPHS = {"ops": (ops_graph, N_OPS), "layers": (lambda: R.GRAPHS["random"][:2], R.N_NODES)}
_ADJACENCIES = {}


class Env:
    """One case on one view: ``view`` the TiledAdjacency view, ``axis`` "row" / "col" for the NumPy models, ``src`` / ``dst`` the edge
    list, and seeded draws. The adjacency of a graph is packed once per process and shared: nothing edits it."""

    def __init__(self, torch, qgtc, case, view_name):
        self.torch, self.Q, self.case, self.view_name = torch, qgtc, case, view_name
        graph = "layers" if case.name.startswith("layer-") else "ops"
        edges, self.n = GRAPHS[graph]
        if graph not in _ADJACENCIES:
            src, dst = edges()
            adj = qgtc.pack_edges_tiled(torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda(), self.n)
            _ADJACENCIES[graph] = (src, dst, adj)
        self.src, self.dst, self.adj = _ADJACENCIES[graph]
        self.view = self.adj.T if view_name == "adj.T" else self.adj
        self.axis = "col" if view_name == "adj.T" else "row"
        self.N, self.H = WIDTH, HEADS

    def rng(self, key):
        return np.random.default_rng([zlib.crc32(self.case.name.encode()), zlib.crc32(key.encode()), VIEWS.index(self.view_name)])

    def draw(self, key, *shape, scale=1.0):
        return self.torch.from_numpy((self.rng(key).standard_normal(shape) * scale).astype(np.float32)).cuda()

    def positive(self, key, *shape):
        return self.torch.from_numpy(self.rng(key).uniform(0.5, 1.5, shape).astype(np.float32)).cuda()

    def flags(self, key, p):
        return self.rng(key).random(self.n) < p

    def bitmap(self, flags):
        from qgtc_ppopp22_amd.tiled import node_bitmap

        return node_bitmap(self.torch.from_numpy(np.asarray(flags, dtype=bool)).cuda(), self.n)

    @property
    def nnz(self):
        from qgtc_ppopp22_amd.tiled import edge_endpoints

        return edge_endpoints(self.view)[0].numel()


# ---- tiledAggregate: sum, max / min, attn ---------------------------------------------------------------------------------------------

def _aggregate(mode, scales=False, drop=False, masks=False, fanout=None):
    """The builder of a ``tiledAggregate`` row. ``fanout``: "pair" (k, seed); "own" / "other" a FanoutSample taken on this view / on the
    other one; "masked" a sample of ``sample_fanout(view, k, seed, row_mask=, nbr_mask=)``, with its own mean as the row scale of the sum."""

    def build(E):
        from qgtc_ppopp22_amd.fanout import sample_fanout

        torch, Q = E.torch, E.Q
        leaves, sides, fixed = {"X": E.draw("X", E.n, E.N)}, {}, {}
        if mode.startswith("attn"):
            shape = (E.n, E.H) if mode == "attn-heads" else (E.n,)
            leaves["attn[0]"], leaves["attn[1]"] = E.draw("p", *shape), E.draw("q", *shape)
        elif mode in ("max", "min"):
            fixed["reduce"] = mode
        if scales:
            sides["row_scale"], sides["src_scale"] = E.positive("r", E.n), E.positive("c", E.n)
        if masks:
            sides["row_mask"], sides["nbr_mask"] = E.bitmap(E.flags("rows", 0.6)), E.bitmap(E.flags("nbrs", 0.5))
        if drop:
            fixed["edge_drop"] = (0.5, SEED)
        sample = None
        if fanout == "pair":
            fixed["fanout"] = (FANOUT_K, SEED)
        elif fanout in ("own", "other"):
            sample = sample_fanout(E.view if fanout == "own" else E.view.T, FANOUT_K, SEED)
        elif fanout == "masked":
            sample = sample_fanout(E.view, FANOUT_K, SEED, row_mask=E.bitmap(E.flags("rows", 0.6)), nbr_mask=E.bitmap(E.flags("nbrs", 0.5)))
            sides.update({"fanout.row_mask": sample.row_mask, "fanout.nbr_mask": sample.nbr_mask, "fanout.counts": sample.counts})
        if sample is not None:
            sides["fanout.thr"] = sample.thr
            fixed["fanout"] = sample

        def keywords():
            kw = dict(fixed, **{k: v for k, v in sides.items() if not k.startswith("fanout.")})
            if fanout == "masked" and mode == "sum":
                kw["row_scale"] = sample.mean_scale()       # reads counts now, as sage.SAGEConv(block=) does
            return kw

        def run(t):
            kw = keywords()
            if mode.startswith("attn"):
                kw["attn"] = (t["attn[0]"], t["attn[1]"])
            return Q.tiledAggregate(E.view, t["X"], **kw)

        second = (lambda Rm: Q.tiledMMFloat(E.view, Rm, **keywords())) if mode == "sum" else None
        return Live(torch, leaves, run, sides, second=second)

    return build


_MASKED_SAMPLE = ("fanout.thr", "fanout.row_mask", "fanout.nbr_mask", "fanout.counts")
_SUM_SPEC = "tiledMMFloat on the view, on the other view for dX (tests/tiled_float_model.py, tiled_sym_model.py, tiled_drop_model.py, tiled_nodes_model.py, tiled_fanout_model.py)"
for _name, _sides, _opt in (("plain", (), {}),
                            ("scales", ("row_scale", "src_scale"), dict(scales=True)),
                            ("edge_drop", (), dict(drop=True)),
                            ("masks-scales", ("row_scale", "src_scale", "row_mask", "nbr_mask"), dict(scales=True, masks=True)),
                            ("fanout-pair", (), dict(fanout="pair")),
                            ("fanout-own", ("fanout.thr",), dict(fanout="own")),
                            ("fanout-other", ("fanout.thr",), dict(fanout="other")),
                            ("fanout-masked", _MASKED_SAMPLE, dict(fanout="masked"))):
    case(f"sum-{_name}", ["_TiledAggregate"], ["X"], _sides, "value", _SUM_SPEC, _aggregate("sum", **_opt))

for _mode in ("max", "min"):
    for _name, _sides, _opt in (("plain", (), {}), ("edge_drop", (), dict(drop=True)), ("masks", ("row_mask", "nbr_mask"), dict(masks=True)),
                                ("fanout-own", ("fanout.thr",), dict(fanout="own"))):
        case(f"{_mode}-{_name}", ["_TiledExtremum"], ["X"], _sides, "raises", "the winners' words and the select (tests/tiled_max_model.py)",
             _aggregate(_mode, **_opt))

_ATT = ["X", "attn[0]", "attn[1]"]
for _name, _sides, _opt in (("plain", (), {}), ("edge_drop", (), dict(drop=True)), ("masks", ("row_mask", "nbr_mask"), dict(masks=True)),
                            ("fanout-own", ("fanout.thr",), dict(fanout="own"))):
    case(f"attn-{_name}", ["_TiledAttention"], _ATT, _sides, "raises", "the fixed float32 sequence of tests/tiled_attn_model.py",
         _aggregate("attn", **_opt))
for _name, _sides, _opt in (("plain", (), {}), ("edge_drop", (), dict(drop=True)), ("masks", ("row_mask", "nbr_mask"), dict(masks=True))):
    case(f"attn-heads-{_name}", ["_TiledAttention"], _ATT, _sides, "raises", "every head the one-head call (tests/tiled_attn_heads_model.py)",
         _aggregate("attn-heads", **_opt))


# ---- edge weights and the edge operators ------------------------------------------------------------------------------------------------

def _weighted(heads, scaled):
    def build(E):
        leaves = {"X": E.draw("X", E.n, E.N), "edge_weight": E.draw("w", *((E.nnz, E.H) if heads else (E.nnz,)))}
        sides = {"row_scale": E.positive("r", E.n)} if scaled else {}
        return Live(E.torch, leaves, lambda t: E.Q.tiledAggregate(E.view, t["X"], edge_weight=t["edge_weight"], **sides), sides)

    return build


_EDGE_SPEC = "the weighted sum and the SDDMM of tests/tiled_edge_model.py, tiled_heads_model.py"
case("edge_weight", ["_TiledWeighted"], ["X", "edge_weight"], (), "raises", _EDGE_SPEC, _weighted(False, False))
case("edge_weight-heads", ["_TiledWeighted"], ["X", "edge_weight"], (), "raises", _EDGE_SPEC, _weighted(True, False))
case("edge_weight-row_scale", ["_TiledWeighted"], ["X", "edge_weight"], ("row_scale",), "raises", _EDGE_SPEC, _weighted(False, True))


def _edge_op(which, heads):
    def build(E):
        from qgtc_ppopp22_amd import tiled

        d, v, h = 2 * 6, E.N, E.H if heads else 1      # d: the width of the scored operands, v: of the values; both divisible by H
        if which == "softmax":
            leaves = {"logits": E.draw("l", *((E.nnz, E.H) if heads else (E.nnz,)))}
            run = lambda t: tiled.tiledEdgeSoftmax(E.view, t["logits"])
        elif which == "scores":
            leaves = {"A": E.draw("A", E.n, d), "B": E.draw("B", E.n, d)}
            run = lambda t: tiled.tiledEdgeScores(E.view, t["A"], t["B"], heads=h)
        elif which == "attention":
            leaves = {"Q": E.draw("Q", E.n, d), "K": E.draw("K", E.n, d), "V": E.draw("V", E.n, v)}
            run = lambda t: tiled.tiledEdgeAttention(E.view, t["Q"], t["K"], t["V"], heads=h)
        elif which == "addscores":
            leaves = {"own": E.draw("own", E.n, d), "nbr": E.draw("nbr", E.n, d), "att": E.draw("att", h, d // h)}
            run = lambda t: tiled.tiledEdgeAdditiveScores(E.view, t["own"], t["nbr"], t["att"], 0.2, heads=h)
        else:
            leaves = {"own": E.draw("own", E.n, d), "nbr": E.draw("nbr", E.n, d), "V": E.draw("V", E.n, v), "att": E.draw("att", h, d // h)}
            run = lambda t: tiled.tiledEdgeAdditiveAttention(E.view, t["own"], t["nbr"], t["V"], t["att"], 0.2, heads=h)
        return Live(E.torch, leaves, run)

    return build


case("edge_softmax", ["_TiledEdgeSoftmax"], ["logits"], (), "raises", "tests/tiled_esoftmax_model.py", _edge_op("softmax", False))
case("edge_softmax-heads", ["_TiledEdgeSoftmax"], ["logits"], (), "raises", "tests/tiled_heads_model.py", _edge_op("softmax", True))
case("edge_scores", ["_TiledEdgeScores"], ["A", "B"], (), "raises", "tests/tiled_edge_model.py", _edge_op("scores", False))
case("edge_scores-heads", ["_TiledEdgeScores"], ["A", "B"], (), "raises", "tests/tiled_heads_model.py", _edge_op("scores", True))
case("edge_attention", ["_TiledEdgeScores", "_TiledEdgeSoftmax", "_TiledWeighted"], ["Q", "K", "V"], (), "raises",
     "the composition of the three (tests/tiled_heads_model.py)", _edge_op("attention", True))
case("edge_additive_scores", ["_TiledEdgeAdditiveScores"], ["own", "nbr", "att"], (), "raises", "tests/tiled_addscore_model.py",
     _edge_op("addscores", True))
case("edge_additive_attention", ["_TiledEdgeAdditiveScores", "_TiledEdgeSoftmax", "_TiledWeighted"], ["own", "nbr", "V", "att"], (), "raises",
     "the composition of the three (tests/tiled_addscore_model.py)", _edge_op("addattention", True))


# ---- layers, at the sizes and parameters of tests/layers_reference.py ----------------------------------------------------------------

def _fill(E, module):
    """Seeded parameters, scaled as the constructors scale theirs; {name: parameter}."""
    torch = E.torch
    params = dict(module.named_parameters())
    with torch.no_grad():
        for name, p in params.items():
            p.copy_(E.draw(name, *p.shape, scale=1.0 / max(p.shape[-1] if name.startswith("lin_") else p.shape[0], 1) ** 0.5))
    return params


def _f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _gcn(drop):
    def build(E):
        from qgtc_ppopp22_amd.conv import GCNConv

        layer = GCNConv(R.F_IN, R.HIDDEN, R.CLASSES, norm="sym", edge_drop=R.DROP_RATE if drop else 0.0).cuda().train()
        params = _fill(E, layer)
        leaves = dict({"X": E.draw("X", E.n, R.F_IN)}, **params)

        def dense(Rm, dtype):
            # the layer pair is linear in X: d<dX, R>/d(dY) is the layer on R
            zero = np.zeros((E.n, R.CLASSES))
            return R.gcn_layer(E.src, E.dst, E.n, _f64(Rm), _f64(layer.W_in), _f64(layer.W_out), zero, view=E.view_name, norm="sym",
                               edge_drop=(R.DROP_RATE, R.DROP_SEED, None) if drop else None, dtype=dtype)["Y"]

        run = lambda t: layer(E.view, t["X"], edge_seed=R.DROP_SEED if drop else None)
        drawn = (lambda t: layer(E.view, t["X"])) if drop else None        # edge_seed=None: 64 bits from torch's CPU generator
        return Live(E.torch, leaves, run, dense=dense, drawn=drawn)

    return build


def _attention_layer(which):
    def build(E):
        from qgtc_ppopp22_amd import conv

        make = {"gat": lambda: conv.GATConv(R.F_IN, R.GAT_OUT, heads=HEADS), "gatv2": lambda: conv.GATv2Conv(R.F_IN, R.GAT_OUT, heads=HEADS),
                "transformer": lambda: conv.TransformerConv(R.F_IN, R.GAT_OUT, heads=HEADS)}[which]
        layer = make().cuda().train()
        leaves = dict({"X": E.draw("X", E.n, R.F_IN)}, **_fill(E, layer))
        return Live(E.torch, leaves, lambda t: layer(E.view, t["X"]))

    return build


def _sage_block():
    def build(E):
        import torch

        from qgtc_ppopp22_amd import fanout, sage

        seeds = np.zeros(E.n, dtype=bool)
        seeds[E.rng("seeds").permutation(E.n)[:BATCH]] = True
        block = fanout.sample_blocks(E.view, E.bitmap(seeds), (FANOUT_K,), SEED)[0]
        layer = sage.SAGEConv(R.F_IN, R.HIDDEN, aggr="mean").cuda().train()
        leaves = dict({"X": E.draw("X", E.n, R.F_IN)}, **_fill(E, layer))
        sides = {"fanout.thr": block.sample.thr, "fanout.row_mask": block.sample.row_mask, "fanout.counts": block.sample.counts}

        def dense(Rm, dtype):
            # linear in X: d<dX, R>/d(dY) is the layer on R without the bias, the mean over the block's kept edges
            ks, kd = bm.kept_edges(E.src, E.dst, E.n, FANOUT_K, block.sample.seed, E.axis, seeds)
            A = torch.zeros((E.n, E.n), dtype=dtype)
            A[torch.from_numpy(ks if E.axis == "row" else kd), torch.from_numpy(kd if E.axis == "row" else ks)] = 1
            deg = A.sum(dim=1)
            Rm, Ws, Wn = (torch.from_numpy(_f64(t)).to(dtype) for t in (Rm, layer.lin_self.weight, layer.lin_nbr.weight))
            mean = (A @ Rm) * torch.where(deg > 0, 1 / deg.clamp(min=1), torch.zeros((), dtype=dtype))[:, None]
            return Rm @ Ws.t() + mean @ Wn.t()

        return Live(E.torch, leaves, lambda t: layer(E.view, t["X"], block=block), sides, dense=dense)

    return build


def _gcn_qnt():
    def build(E):
        from qgtc_ppopp22_amd.conv import GCNConv_Qnt

        layer = GCNConv_Qnt(48, 64, 10, w_bit=2, act_bit=3).cuda()
        A = E.torch.from_numpy(R.dense_adjacency(E.src, E.dst, E.n, E.view_name).astype(np.float32)).cuda()
        leaves = dict({"X": E.draw("X", E.n, 48).abs()}, **dict(layer.named_parameters()))
        return Live(E.torch, leaves, lambda t: layer(A, t["X"]))

    return build


_GCN, _LAYER_SPEC = ["X", "W_in", "W_out"], "the dense float64 definition of tests/layers_reference.py, within its tolerances"
case("layer-gcn-sym", ["_TiledAggregate"], _GCN, (), "dense", _LAYER_SPEC, _gcn(False))
case("layer-gcn-sym-edge_drop", ["_TiledAggregate"], _GCN, (), "dense", _LAYER_SPEC, _gcn(True))
case("layer-gat-heads", ["_TiledAttention"], ["X", "W", "a_dst", "a_src"], (), "raises", _LAYER_SPEC, _attention_layer("gat"))
case("layer-gatv2", ["_TiledEdgeAdditiveScores", "_TiledEdgeSoftmax", "_TiledWeighted"], ["X", "W_l", "W_r", "att"], (), "raises",
     "the dense definition in tests/test_gatv2_dense_gpu.py", _attention_layer("gatv2"))
case("layer-transformer", ["_TiledEdgeScores", "_TiledEdgeSoftmax", "_TiledWeighted"], ["X", "W_q", "W_k", "W_v"], (), "raises",
     "tests/transformer_reference.py", _attention_layer("transformer"))
case("layer-sage-mean-block", ["_TiledAggregate"], ["X", "lin_self.weight", "lin_self.bias", "lin_nbr.weight"],
     ("fanout.thr", "fanout.row_mask", "fanout.counts"), "dense", "the dense mean over the block's kept edges (tests/tiled_blocks_model.py)",
     _sage_block())
case("layer-gcn-qnt", ["Aggregation_Qnt"], ["X", "W_in", "W_out"], (), "inference", "the CPU oracle's words (tests/test_gpu_extras.py)", _gcn_qnt())

DIFFERENTIABLE = [c for c in CASES if c.second != "inference"]

# Rows whose output is formed by torch operators AFTER the package's Function: no form of dY ever reaches the Function (its incoming
# gradient is the fresh, contiguous result of torch.nn.Linear's backward), while torch's own GEMMs pick their kernels, and with them
# their rounding, by the strides of dY. The forms-of-dY property says nothing about this package there and is not run on them.
DY_MEETS_TORCH_FIRST = ("layer-sage-mean-block",)
