"""The table of the module-state tests (tests/test_module_state.py on the CPU, tests/test_module_state_gpu.py on the device): every
``torch.nn.Module`` of qgtc_ppopp22_amd/conv.py and sage.py as a long-lived object - trained, reloaded, copied, re-configured, switched
between ``train()`` and ``eval()`` and moved between graphs.

A ROW carries a name, the class, the hyper-parameters it is built with (``make(**hyper)``), the names of its parameters (``params``),
one forward (``call(layer, A, X, seed)``, A a :class:`Form`), the classification of every attribute the class assigns that is neither a
Parameter nor a sub-module (``attributes``, shared by the rows of a class: ``ATTRIBUTES``), the values property 2 assigns to its "hyper"
attributes (``reconfigure``) and the independent definition it is anchored to (``reference``, evaluated by :func:`reference`).

``attributes`` kinds:  "hyper"    read at every forward, may be reassigned;
                       "derived"  computed from another attribute, which it follows;
                       "cache"    a tensor kept between forwards, with the key it is valid for;
                       "fixed"    a shape (it sizes the parameters or decides which exist): not reassignable.

``WRITE_ROUTES`` are the ways torch offers to change a parameter, each a function ``(layer, new_values) -> layer`` (``new_values``
{name: float32 numpy}; the optimiser routes and ``half().float()`` end at values of their own, read back from the layer), with two
flags that tests/test_module_state.py holds against a plain ``torch.nn.Linear``: whether the route changes ``weight._version`` and
whether it replaces the Parameter object. Five routes change neither, so no key made of versions and identities can tell that the
weights moved: GCNConv_Qnt packs its weights in every forward.

Widths are those of tests/layers_reference.py (F_IN, HIDDEN, CLASSES, GAT_OUT), 2 heads. Graphs: its dyadic and random graph (N_NODES
nodes) and ``SECOND``, a random graph of another size. Importing this module needs neither a GPU nor the built extension."""
import numpy as np

import layers_reference as R
from tiled_model import random_edges

HEADS = 2
W_BIT, ACT_BIT = 2, 6                         # requant clamps above 2^6: with 3 bits the sums over 16 neighbours all clamp (see features)
BLOCK_K = 4                                   # the block row's fanout: on the dyadic graph 0, 1 or 4 kept neighbours, so the mean is exact
SEED, OTHER_SEED = R.DROP_SEED, 0x0F1E2D3C4B5A6978
N_SECOND = 200                                # 7 row blocks and 2 k-quads, both ragged
KINDS = ("hyper", "derived", "cache", "fixed")

ATTRIBUTES = {
    "GCNConv_Qnt": {"aggr": ("hyper", ""), "float_out": ("hyper", ""), "w_bit": ("hyper", ""), "act_bit": ("hyper", ""),
                    "validate_edges": ("hyper", "edge-list adjacencies only"),
                    "input_dim": ("fixed", ""), "hidden_dim": ("fixed", ""), "output_dim": ("fixed", ""),
                    "bit_W_in": ("cache", "none: every forward packs it again from W_in and w_bit"),
                    "bit_W_out": ("cache", "none: every forward packs it again from W_out and w_bit")},
    "GCNConv": {"edge_drop": ("hyper", ""), "norm": ("hyper", ""), "aggr": ("hyper", ""),
                "_edge_drop": ("derived", "edge_drop as its setter checked it: the property's storage"),
                "keep_scale": ("derived", "float32(1 / (1 - edge_drop))"),
                "_keep_vector": ("cache", "(n, device, keep_scale)")},
    "GATConv": {"edge_drop": ("hyper", ""), "negative_slope": ("hyper", ""), "concat": ("hyper", ""),
                "input_dim": ("fixed", ""), "output_dim": ("fixed", ""), "heads": ("fixed", "")},
    "TransformerConv": {"concat": ("hyper", ""), "input_dim": ("fixed", ""), "output_dim": ("fixed", ""), "heads": ("fixed", "")},
    "GATv2Conv": {"negative_slope": ("hyper", ""), "concat": ("hyper", ""), "input_dim": ("fixed", ""), "output_dim": ("fixed", ""),
                  "heads": ("fixed", ""), "share_weights": ("fixed", "decides whether W_r exists")},
    "SAGEConv": {"aggr": ("hyper", ""), "fanout": ("hyper", "")},
}
MODULES = {"SAGEConv": ("lin_self", "lin_nbr")}    # sub-modules, by class: their parameters are named with the dot
FILES = {"GCNConv_Qnt": "conv", "GCNConv": "conv", "GATConv": "conv", "TransformerConv": "conv", "GATv2Conv": "conv", "SAGEConv": "sage"}
_DIMS = {"GCNConv_Qnt": (R.F_IN, R.HIDDEN, R.CLASSES), "GCNConv": (R.F_IN, R.HIDDEN, R.CLASSES), "GATConv": (R.F_IN, R.GAT_OUT),
         "TransformerConv": (R.F_IN, R.GAT_OUT), "GATv2Conv": (R.F_IN, R.GAT_OUT), "SAGEConv": (R.F_IN, R.HIDDEN)}

SECOND = random_edges(np.random.default_rng(2026), N_SECOND, 6 * N_SECOND)
GRAPHS = {"dyadic": R.GRAPHS["dyadic"][:2] + (R.N_NODES,), "random": R.GRAPHS["random"][:2] + (R.N_NODES,),
          "second": (SECOND[0], SECOND[1], N_SECOND)}


class Form:
    """One adjacency form of one graph: ``adj`` the TiledAdjacency view, ``view`` "adj" / "adj.T", ``rank`` (numpy, rank[old] = new) or
    None without reorder, the edge list, and ``dense`` - the float32 0/1 matrix of the view in the edge list's numbering (a device
    tensor, built on first use) for the rows that take a dense A."""

    def __init__(self, graph, label, adj, view, rank):
        self.graph, self.label, self.adj, self.view, self.rank = graph, label, adj, view, rank
        self.src, self.dst, self.n = GRAPHS[graph]
        self._dense = None

    def __repr__(self):
        return f"{self.graph} {self.label}"

    @property
    def dense(self):
        if self._dense is None:
            import torch

            self._dense = torch.from_numpy(R.dense_adjacency(self.src, self.dst, self.n, self.view).astype(np.float32)).to(self.adj.device)
        return self._dense


def forms(torch, qgtc, graph):
    """[plain adj, adj.T, reordered adj, reordered adj.T] of a graph, as tests/test_layers_dense_gpu.py::forms builds them."""
    src, dst, n = GRAPHS[graph]
    s, d = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
    plain = qgtc.pack_edges_tiled(s, d, n)
    moved = qgtc.pack_edges_tiled(s, d, n, reorder=True)
    assert plain.perm is None and moved.perm is not None
    rank = moved.rank.cpu().numpy()
    return [Form(graph, "adj", plain, "adj", None), Form(graph, "adj.T", plain.T, "adj.T", None),
            Form(graph, "reordered adj", moved, "adj", rank), Form(graph, "reordered adj.T", moved.T, "adj.T", rank)]


def batch_flags(n):
    """bool [n]: the seed nodes of the block row's mini-batch, in the edge list's numbering (layers_reference.batch_flags)."""
    return R.batch_flags(n)


def block_of(A):
    """The one-hop ``fanout.Block`` of the block row on the form ``A``: sampled on A's view from the moved seed flags."""
    import torch

    from qgtc_ppopp22_amd import fanout
    from qgtc_ppopp22_amd.tiled import node_bitmap

    flags = torch.from_numpy(batch_flags(A.n)).to(A.adj.device)
    return fanout.sample_blocks(A.adj, node_bitmap(A.adj.to_new(flags), A.n), (BLOCK_K,), SEED)[0]


class Row:
    def __init__(self, name, cls, hyper, params, how, reference, exact, reconfigure):
        assert how in ("qnt-dense", "qnt-tiled", "edge_seed", "plain", "seed", "block")
        self.name, self.cls, self.hyper, self.params, self.how = name, cls, dict(hyper), tuple(params), how
        self.reference, self.exact, self.reconfigure = reference, exact, dict(reconfigure)
        self.attributes = ATTRIBUTES[cls]
        self.modules = MODULES.get(cls, ())

    def __repr__(self):
        return self.name

    @property
    def quantised(self):
        return self.cls == "GCNConv_Qnt"

    @property
    def graph(self):
        """The graph the row is anchored on: the dyadic one where its definition is exact in float32, else the random one."""
        return "dyadic" if self.exact else "random"

    @property
    def sampling(self):
        """The hyper-parameter whose value makes ``train()`` sample, or None."""
        for name in ("edge_drop", "fanout"):
            if self.hyper.get(name):
                return name
        return None

    def make(self, **hyper):
        """A new layer on the CPU with the row's hyper-parameters, ``hyper`` over them. A hyper attribute the constructor does not take
        (``validate_edges``) is assigned right after it, before any call."""
        import importlib
        import inspect

        cls = getattr(importlib.import_module(f"qgtc_ppopp22_amd.{FILES[self.cls]}"), self.cls)
        kw = dict(self.hyper, **hyper)
        if self.cls in ("GATConv", "TransformerConv", "GATv2Conv"):
            kw.setdefault("heads", HEADS)
        taken = inspect.signature(cls.__init__).parameters
        later = {k: kw.pop(k) for k in list(kw) if k not in taken}
        assert all(self.attributes[k][0] == "hyper" for k in later), later
        layer = cls(*_DIMS[self.cls], **kw)
        for k, v in later.items():
            setattr(layer, k, v)
        return layer

    def call(self, layer, A, X, seed=None):
        """One forward of ``layer`` on the form ``A``; ``seed`` reaches the layers that sample."""
        if self.how == "qnt-dense":
            return layer(A.dense, X)
        if self.how in ("qnt-tiled", "plain"):
            return layer(A.adj, X)
        if self.how == "edge_seed":
            return layer(A.adj, X, edge_seed=seed)
        if self.how == "seed":
            return layer(A.adj, X, seed=seed)
        return layer(A.adj, X, block=block_of(A))

    def out_width(self, layer):
        if self.cls in ("GCNConv_Qnt", "GCNConv"):
            return R.CLASSES
        if self.cls == "SAGEConv":
            return R.HIDDEN
        return HEADS * R.GAT_OUT if layer.concat else R.GAT_OUT


_GCN_REF = "layers_reference.gcn_layer, dense float64"
_QNT_REF = "the integer NumPy chain over np_quantize / np_requant (tests/test_gpu_extras.py), on the tiled models for mean and float_out"
_DROP = {"edge_drop": (0.5, 0.0)}
_QNT = {"w_bit": (3,), "act_bit": (3,), "float_out": (True,), "aggr": ("mean",), "validate_edges": (False,)}
_QNT_HYPER = {"w_bit": W_BIT, "act_bit": ACT_BIT}
_SAGE = ("lin_self.weight", "lin_self.bias", "lin_nbr.weight")

ROWS = [
    Row("qnt-dense", "GCNConv_Qnt", _QNT_HYPER, ("W_in", "W_out"), "qnt-dense", _QNT_REF, True, _QNT),
    Row("qnt-tiled-sum", "GCNConv_Qnt", _QNT_HYPER, ("W_in", "W_out"), "qnt-tiled", _QNT_REF, True, _QNT),
    Row("qnt-tiled-mean", "GCNConv_Qnt", dict(_QNT_HYPER, aggr="mean"), ("W_in", "W_out"), "qnt-tiled", _QNT_REF, True,
        dict(_QNT, aggr=("sum",))),
    Row("qnt-float_out", "GCNConv_Qnt", dict(_QNT_HYPER, float_out=True), ("W_in", "W_out"), "qnt-tiled", _QNT_REF, True,
        dict(_QNT, float_out=(False,))),
    # keep_scale = float32(4 / 3) is no power of two: the sums round in float32, so these two are held within the tolerances
    Row("gcn-None-drop", "GCNConv", dict(norm=None, edge_drop=0.25), ("W_in", "W_out"), "edge_seed", _GCN_REF, False,
        dict(_DROP, norm=("sym", "mean"), aggr=("max",))),
    Row("gcn-sym-drop", "GCNConv", dict(norm="sym", edge_drop=0.25), ("W_in", "W_out"), "edge_seed", _GCN_REF, False,
        dict(_DROP, norm=(None,), aggr=("max",))),      # "max" beside norm="sym" is no layer: refused
    Row("gcn-max-drop", "GCNConv", dict(aggr="max", edge_drop=0.25), ("W_in", "W_out"), "edge_seed", _GCN_REF, True,
        dict(_DROP, norm=("sym",), aggr=("sum", "min"))),
    Row("gat", "GATConv", {}, ("W", "a_dst", "a_src"), "edge_seed", "layers_reference.gat_layer, dense float64", False,
        {"edge_drop": (0.5,), "negative_slope": (0.5,), "concat": (False,)}),
    Row("gat-drop", "GATConv", dict(edge_drop=0.25), ("W", "a_dst", "a_src"), "edge_seed", "layers_reference.gat_layer, dense float64",
        False, dict(_DROP, negative_slope=(0.5,), concat=(False,))),
    Row("gatv2", "GATv2Conv", {}, ("W_l", "W_r", "att"), "plain", "gatv2_reference.gatv2_layer, dense float64", False,
        {"negative_slope": (0.5,), "concat": (False,)}),
    Row("gatv2-shared", "GATv2Conv", dict(share_weights=True), ("W_l", "att"), "plain", "gatv2_reference.gatv2_layer(shared=True)",
        False, {"negative_slope": (0.5,), "concat": (False,)}),
    Row("transformer", "TransformerConv", {}, ("W_q", "W_k", "W_v"), "plain", "transformer_reference.transformer_layer, dense float64",
        False, {"concat": (False,)}),
    # min(deg, 3) is 3 on most nodes of the dyadic graph: 1 / 3 rounds, so the fanout row is held within the tolerances
    Row("sage-fanout", "SAGEConv", dict(fanout=3), _SAGE, "seed", "layers_reference.sage_layer(fanout=3), dense float64", False,
        {"fanout": (5, None), "aggr": ("max",)}),
    Row("sage-block", "SAGEConv", {}, _SAGE, "block", "layers_reference.sage_layer over the block's kept edges, dense float64", True,
        {"fanout": (3,), "aggr": ("max",)}),
]
BY_NAME = {r.name: r for r in ROWS}
assert len(BY_NAME) == len(ROWS)


# ---- values -------------------------------------------------------------------------------------------------------------------------

def _rng(row, what, k=0):
    import zlib

    return np.random.default_rng([zlib.crc32(row.name.encode()), zlib.crc32(what.encode()), k])


def shapes(layer, row):
    named = dict(layer.named_parameters())
    return {name: tuple(named[name].shape) for name in row.params}


# float32 values beside a rounding tie of the weight quantiser, by the code they have and the code after a trip through float16 (which
# lands them on the tie; ties go to the even code): 0.25 and 2.0 keep theirs, the other four change it. Codes 0 and 2 cannot change.
_TIES = np.array([0.25, 2.0, 0.5 + 2.0 ** -14, 1.5 - 2.0 ** -13, 2.5 + 2.0 ** -12, 3.5 - 2.0 ** -12], dtype=np.float32)
_TIE_SHARE = [0.30, 0.10, 0.25, 0.20, 0.10, 0.05]      # 60 % of the elements change their code under half().float()


def old_values(row, layer):
    """{name: float32 numpy}: the values a layer holds while it warms up. Quantised rows: values beside the quantiser's ties (see
    _TIES). Float rows: standard normal, scaled as the constructors scale theirs - no integers, so that float16 rounds them."""
    out = {}
    for name, shape in shapes(layer, row).items():
        rng = _rng(row, "old " + name)
        if row.quantised:
            out[name] = _TIES[rng.choice(len(_TIES), size=shape, p=_TIE_SHARE)]
        else:
            fan = shape[-1] if name.startswith("lin_") else shape[0]
            out[name] = (rng.standard_normal(shape) / max(fan, 1) ** 0.5).astype(np.float32)
    return out


def new_values(row, layer, k=1):
    """{name: float32 numpy}: the values a write route is given. Quantised rows: every element's code differs from the code of
    :func:`old_values` (old + 1 or + 2 modulo 4), the value well inside the code's interval. Exact float rows: small integers (the dense
    definition is then exact in float32 on the dyadic graph). Other float rows: another standard-normal draw."""
    from oracle.qgtc_oracle import np_quantize

    out = {}
    old = old_values(row, layer)
    for name, shape in shapes(layer, row).items():
        rng = _rng(row, "new " + name, k)
        if row.quantised:
            code = (codes(old[name], W_BIT) + rng.integers(1, 3, size=shape)) % (1 << W_BIT)
            out[name] = (code + rng.uniform(0.0, 0.3, size=shape)).astype(np.float32)
            assert (codes(out[name], W_BIT) == code).all() and np_quantize(out[name], W_BIT).max() < (1 << W_BIT)
        elif row.exact:
            out[name] = rng.integers(-2, 3, size=shape).astype(np.float32)
        else:
            fan = shape[-1] if name.startswith("lin_") else shape[0]
            out[name] = (rng.standard_normal(shape) / max(fan, 1) ** 0.5).astype(np.float32)
    return out


def codes(values, bits):
    """int64: the codes the quantiser packs for ``values`` - np_quantize, its low ``bits`` bits."""
    from oracle.qgtc_oracle import np_quantize

    return np_quantize(np.asarray(values, dtype=np.float32), bits).astype(np.int64) & ((1 << bits) - 1)


def features(row, n, k=0, integer=False):
    """float32 [n, F_IN]: the node features. Quantised rows: one element in fifty holds code 1 or 2 and the others 0 - denser
    inputs run every product into requant's clamp, and the output stops depending on the weights. Float rows: standard normal, or small
    integers for the exact anchor."""
    rng = _rng(row, "X", k)
    if row.quantised:
        x = np.where(rng.random((n, R.F_IN)) < 0.02, rng.integers(1, 3, size=(n, R.F_IN)), 0) + rng.uniform(0.0, 0.3, size=(n, R.F_IN))
        return x.astype(np.float32)
    if integer:
        return rng.integers(-3, 4, size=(n, R.F_IN)).astype(np.float32)
    return rng.standard_normal((n, R.F_IN)).astype(np.float32)


# ---- the independent definitions ------------------------------------------------------------------------------------------------------

def qnt_chain(oracle, src, dst, n, X, Wi, Wo, transposed, aggr, float_out, w_bit=W_BIT, act_bit=ACT_BIT):
    """GCNConv_Qnt in integers on the quantised adjacency of an edge list (``transposed``: of its other view), as
    tests/test_gpu_extras.py and tests/test_capture_modules_gpu.py::qnt_model write it: A . rq(rq(A . rq(qX . qW_in)) . qW_out), with the
    float32 epilogues of the tiled models for ``aggr="mean"`` and ``float_out``."""
    from oracle.qgtc_oracle import np_requant
    from tiled_float_model import aggregate_f32
    from tiled_model import aggregate
    from tiled_scaled_model import degrees, mean_scale, scaled

    low = lambda q, b: np.asarray(q).astype(np.int64) & ((1 << b) - 1)      # noqa: E731
    rq = lambda c: low(np_requant(np.asarray(c).astype(np.int32), act_bit), act_bit)   # noqa: E731
    qX, qWi, qWo = codes(X, act_bit), codes(Wi, w_bit), codes(Wo, w_bit)
    scale = mean_scale(degrees(src, dst, n)[1 if transposed else 0]) if aggr == "mean" else None
    c1 = aggregate(src, dst, n, rq(qX @ qWi), transposed)
    h = low(oracle.quantize(scaled(c1, scale), act_bit), act_bit) if aggr == "mean" else rq(c1)
    if float_out:
        hw = oracle.bitmm2int(oracle.pack(h, act_bit), oracle.val2bit(np.asarray(Wo, dtype=np.float32), w_bit, True), n, Wo.shape[0],
                              Wo.shape[1], act_bit, w_bit)
        return aggregate_f32(src, dst, n, hw, transposed, scale)
    c2 = aggregate(src, dst, n, rq(h @ qWo), transposed)
    return scaled(c2, scale) if aggr == "mean" else c2.astype(np.float32)


def reference(row, A, X, values, hyper=None, seed=None, dtype_name="float64", oracle=None):
    """float64 numpy: the output the row's independent definition gives on the form ``A`` for the features ``X`` and the parameter
    ``values`` ({name: numpy}), in ``train()`` with the sampling seed ``seed``. The quantised rows return the float32 words' values; the
    block row the batch rows only. ``dtype_name`` "float32" sizes layers_reference.tolerances."""
    import torch

    import gatv2_reference
    import transformer_reference

    o = dict(row.hyper, **(hyper or {}))
    dtype = getattr(torch, dtype_name)
    v = {k: np.asarray(t, dtype=np.float64) for k, t in values.items()}
    X = np.asarray(X, dtype=np.float64)
    src, dst, n = A.src, A.dst, A.n
    if row.cls == "GCNConv_Qnt":
        return qnt_chain(oracle, src, dst, n, X, v["W_in"], v["W_out"], A.view == "adj.T", o.get("aggr", "sum"), o.get("float_out", False),
                         o["w_bit"], o["act_bit"]).astype(np.float64)
    zero = lambda width: np.zeros((n, width))     # noqa: E731
    drop = (o["edge_drop"], seed, A.rank) if o.get("edge_drop") else None
    if row.cls == "GCNConv":
        aggr = o.get("aggr", "sum")
        Y = R.gcn_layer(src, dst, n, X, v["W_in"], v["W_out"], zero(R.CLASSES), view=A.view, norm=o.get("norm"), aggr=aggr, edge_drop=drop,
                        rank=A.rank if aggr != "sum" else None, dtype=dtype)["Y"]
    elif row.cls == "GATConv":
        concat = o.get("concat", True)
        Y = R.gat_layer(src, dst, n, X, v["W"], v["a_dst"], v["a_src"], zero(HEADS * R.GAT_OUT if concat else R.GAT_OUT), view=A.view,
                        heads=HEADS, concat=concat, negative_slope=o.get("negative_slope", 0.2), edge_drop=drop, dtype=dtype)["Y"]
    elif row.cls == "GATv2Conv":
        concat, shared = o.get("concat", True), o.get("share_weights", False)
        Y = gatv2_reference.gatv2_layer(src, dst, n, X, v["W_l"], v["W_l"] if shared else v["W_r"], v["att"],
                                        zero(HEADS * R.GAT_OUT if concat else R.GAT_OUT), view=A.view, heads=HEADS, concat=concat,
                                        slope=o.get("negative_slope", 0.2), shared=shared, dtype=dtype)["Y"]
    elif row.cls == "TransformerConv":
        concat = o.get("concat", True)
        Y = transformer_reference.transformer_layer(src, dst, n, X, v["W_q"], v["W_k"], v["W_v"],
                                                    zero(HEADS * R.GAT_OUT if concat else R.GAT_OUT), view=A.view, heads=HEADS,
                                                    concat=concat, dtype=dtype)["Y"]
    else:
        params = [(v["lin_self.weight"], v["lin_self.bias"], v["lin_nbr.weight"])]
        aggr = o.get("aggr", "mean")
        if row.how == "block":
            Y = R.sage_layer(src, dst, n, X, params, zero(R.HIDDEN), view=A.view, aggr=aggr, fanout=(BLOCK_K,), batch=batch_flags(n),
                             seed=SEED, rank=A.rank, dtype=dtype)["Y"]
        else:
            Y = R.sage_layer(src, dst, n, X, params, zero(R.HIDDEN), view=A.view, aggr=aggr, fanout=o.get("fanout"), seed=seed,
                             rank=A.rank, dtype=dtype)["Y"]
    return Y.to(torch.float64).numpy()


# ---- the write routes -----------------------------------------------------------------------------------------------------------------

def _tensors(layer, new_values):
    import torch

    named = dict(layer.named_parameters())
    return {name: torch.from_numpy(np.ascontiguousarray(v)).to(named[name].device) for name, v in new_values.items()}, named


def _no_grad(layer, new_values):
    import torch

    new, named = _tensors(layer, new_values)
    with torch.no_grad():
        for name, t in new.items():
            named[name].mul_(0.0).add_(t)
    return layer


def _step(make_optimiser):
    def route(layer, new_values):
        new, named = _tensors(layer, new_values)
        for name, t in new.items():
            named[name].grad = named[name].detach() - t      # lr 1: SGD lands beside the new values, Adam one unit towards them
        make_optimiser([named[name] for name in new]).step()
        for p in named.values():
            p.grad = None
        return layer

    return route


def _sgd(layer, new_values):
    import torch

    return _step(lambda ps: torch.optim.SGD(ps, lr=1.0))(layer, new_values)


def _adam(layer, new_values):
    import torch

    return _step(lambda ps: torch.optim.Adam(ps, lr=1.0, foreach=True))(layer, new_values)


def _state(layer, new_values):
    new, _ = _tensors(layer, new_values)
    state = {k: t.clone() for k, t in layer.state_dict().items()}
    state.update(new)
    return state


def _load(layer, new_values):
    layer.load_state_dict(_state(layer, new_values))
    return layer


def _load_assign(layer, new_values):
    layer.load_state_dict(_state(layer, new_values), assign=True)
    return layer


def _data_copy(layer, new_values):
    new, named = _tensors(layer, new_values)
    for name, t in new.items():
        named[name].data.copy_(t)
    return layer


def _data_assign(layer, new_values):
    new, named = _tensors(layer, new_values)
    for name, t in new.items():
        named[name].data = t
    return layer


def _vector(layer, new_values):
    import torch

    new, named = _tensors(layer, new_values)
    vec = torch.cat([(new[name] if name in new else p.detach()).reshape(-1) for name, p in named.items()])
    torch.nn.utils.vector_to_parameters(vec, layer.parameters())
    return layer


def _half_float(layer, new_values):
    return layer.half().float()


def _cpu_and_back(layer, new_values):
    import torch

    device = next(layer.parameters()).device
    layer.cpu()
    named = dict(layer.named_parameters())
    with torch.no_grad():
        for name, v in new_values.items():
            named[name].copy_(torch.from_numpy(np.ascontiguousarray(v)))
    return layer.to(device)


class Route:
    """``write(layer, new_values) -> layer``; ``bumps``: the route changes ``_version`` of the parameter it wrote; ``replaces``: the
    layer holds another Parameter object afterwards; ``given``: the layer ends at ``new_values`` (else at values of the route's own)."""

    def __init__(self, name, write, bumps, replaces, given=True):
        self.name, self.write, self.bumps, self.replaces, self.given = name, write, bumps, replaces, given

    def __repr__(self):
        return self.name


WRITE_ROUTES = [
    Route("no_grad", _no_grad, True, False),
    Route("sgd", _sgd, True, False, given=False),
    Route("adam-foreach", _adam, True, False, given=False),
    Route("load_state_dict", _load, True, False),
    # a new Parameter at version 0: the version a parameter has that was only ever written through .data
    Route("load_state_dict-assign", _load_assign, False, True),
    Route("data.copy_", _data_copy, False, False),
    Route("data=", _data_assign, False, False),
    Route("vector_to_parameters", _vector, False, False),
    Route("half-float", _half_float, False, False, given=False),
    Route("cpu-cuda", _cpu_and_back, True, False),
]
UNSEEN = [r.name for r in WRITE_ROUTES if not r.bumps]     # what torch's version counter does not see
