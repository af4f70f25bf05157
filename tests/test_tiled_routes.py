"""The routes of the family launchers of tiled.py, without a device and without opening the library: for
every (family, heads, view, subgraph kind) the route choice (``tiled._c_route``) and the name rule (``tiled._c_name``) name either a
float binding of the extension or a C entry that one of the six headers declares, exactly where ``tiled._resolve`` lets the call
through; and every entry the attention-with-heads, fanout and blocks headers declare for these families is named by some route. A
typo in a composed name fails here, not on the first call of that combination on a GPU.

"Heads" are the scores' (``attn=`` with [n, H] tensors): the sum and the extremum have none - the columns of X select nothing, and the
attention's shift is the extremum on the [n, H] scores as a matrix -, so for those two families the heads axis changes neither the
call nor the route."""
import inspect
import itertools

import pytest
import torch

import qgtc_ppopp22_amd.tiled as tiled
from qgtc_ppopp22_amd import cabi
from test_tiled_binding_gpu import BINDINGS

N, WORDS = 40, (40 + 127) // 128 * 4
HEADERS = (cabi.HEADER, cabi.HEADS_HEADER, cabi.ATTN_HEADS_HEADER, cabi.ADDSCORE_HEADER, cabi.FANOUT_HEADER, cabi.BLOCKS_HEADER)
FLOAT_BINDINGS = {b for b in BINDINGS if b.startswith("_tiled_mm_f32")}

# family -> (the launcher, the function that holds its C launch, the stem of its C entries, the bindings of its one-head route)
FAMILIES = {"sum": (tiled._sum, tiled._sum, "qgtc_tiledmm_f32", ("_tiled_mm_f32", "_tiled_mm_f32_src")),
            "extremum": (tiled._extremum, tiled._extremum, "qgtc_tiledmax_f32", ("_tiled_mm_f32",)),
            "att_product": (tiled._att_product, tiled._att_heads_product, "qgtc_tiledatt_f32", ("_tiled_mm_f32",)),
            "att_grad": (tiled._att_grad, tiled._att_heads_grad, "qgtc_tiledatt_grad_f32", ("_tiled_mm_f32",))}
HEADS = {"one": 0, "several": 2}
KINDS = ("all", "dropout", "node masks", "sample", "masked sample")


def _declared(*headers):
    names = set()
    for path in headers:
        with open(path) as f:
            names |= set(cabi.signatures(f.read()))
    return names


@pytest.fixture(scope="module")
def views():
    """(adj, adj.T) of CPU tensors without a tile; the other view is put together by hand, as ``adj.T`` would need the device."""
    def one():
        return tiled.TiledAdjacency(N, torch.zeros((N + 31) // 32 + 1, dtype=torch.int64), torch.zeros(0, dtype=torch.int32),
                                    torch.zeros((0, 32, 4), dtype=torch.int32))
    adj, t = one(), one()
    t.transposed, t._other, adj._other = True, adj, t
    return {"row": adj, "column": t}


ROW_MASK, NBR_MASK = torch.zeros(WORDS, dtype=torch.int32), torch.ones(WORDS, dtype=torch.int32)


def _keywords(kind, taken_on):
    """the keywords of a public call under the subgraph kind; a sample is taken (by hand) on the view ``taken_on``"""
    thr = torch.zeros(N, dtype=torch.int32)
    return {"all": {}, "dropout": dict(edge_drop=(0.25, 7)), "node masks": dict(row_mask=ROW_MASK, nbr_mask=NBR_MASK),
            "sample": dict(fanout=tiled.FanoutSample(taken_on, 3, 1, thr)),
            "masked sample": dict(fanout=tiled.FanoutSample(taken_on, 3, 1, thr, ROW_MASK, NBR_MASK, torch.zeros(N, dtype=torch.int32)))}[kind]


def _resolved(adj, family, heads, kw):
    """(mode, subgraph, slope) of the public call that reaches the family, or the ValueError ``_resolve`` refuses it with"""
    H = HEADS[heads] if family.startswith("att") else 0
    X = torch.ones(N, 8)
    call = dict(row_scale=None, src_scale=None, reduce="max" if family == "extremum" else "sum", return_arg=False, attn=None,
                negative_slope=0.2, return_stats=False, edge_drop=None, row_mask=None, nbr_mask=None, edge_weight=None)
    if family.startswith("att"):
        call["attn"] = (torch.zeros((N, H) if H else N), torch.zeros((N, H) if H else N))
    return H, tiled._resolve(adj, X, **{**call, **kw})


def _route(family, H, transposed, sub):
    """("binding", names) or ("entry", name) of one launch"""
    _, _, stem, bindings = FAMILIES[family]
    if tiled._c_route(H, sub):
        return "entry", tiled._c_name(stem, H, transposed, sub)
    assert sub.kw is not None
    return "binding", tuple(tiled._ON_T[b] if transposed else b for b in bindings)


CROSS = list(itertools.product(FAMILIES, HEADS, ("row", "column"), KINDS))


def test_the_launchers_hold_the_stems_and_bindings_of_the_table():
    for family, (launcher, c_launch, stem, bindings) in FAMILIES.items():
        assert f'"{stem}"' in inspect.getsource(c_launch), family
        source = inspect.getsource(launcher) + (inspect.getsource(tiled._att) if family.startswith("att") else "")
        # the sum and the extremum have no heads: they write _c_route(0, sub) out as the test of the subgraph's binding keywords
        assert ("_c_route(att_own.dim() == 2, sub)" if family.startswith("att") else "if sub.kw is not None:") in inspect.getsource(launcher), family
        for b in bindings:
            assert f'"{b}"' in source, (family, b)
        if c_launch is not launcher:
            assert c_launch.__name__ + "(" in inspect.getsource(launcher), family
    assert '"qgtc_rowdot_f32"' in inspect.getsource(tiled._att_heads_rowdot) and "_c_route(" in inspect.getsource(tiled._rowdot)


@pytest.mark.parametrize("family,heads,view,kind", CROSS)
def test_what_resolve_lets_through_has_a_route_and_what_it_refuses_has_none(views, family, heads, view, kind):
    adj = views[view]
    declared = _declared(*HEADERS)
    for taken_on in views.values() if "sample" in kind else (adj,):
        kw = _keywords(kind, taken_on)
        try:
            H, (_, sub, _) = _resolved(adj, family, heads, kw)
        except ValueError as refusal:   # heads with a sample: no route either
            assert "sample" in kind and family.startswith("att") and HEADS[heads] and "[n, H] scores: not built" in str(refusal)
            with pytest.raises(ValueError, match="not built"):
                _route(family, HEADS[heads], adj.transposed, tiled._Subgraph.of(sample=kw["fanout"]))
            continue
        assert (sub is tiled._ALL) == (kind == "all") and tiled._c_route(0, sub) == (sub.kw is None)
        how, names = _route(family, H, adj.transposed, sub)
        if how == "binding":
            assert set(names) <= FLOAT_BINDINGS and not H and "sample" not in kind
            assert set(sub.kw) == {"all": set(), "dropout": {"edge_drop"}, "node masks": {"node_masks"}}[kind]
        else:
            assert names in declared, names
            assert H or "sample" in kind
            assert ("_t_" in names or names.endswith("_t")) == adj.transposed and ("_heads_" in names) == bool(H)
            assert (sub.kw is None) == ("sample" in kind)   # a sample has no binding route


@pytest.mark.parametrize("view", ["row", "column"])
def test_the_combinations_without_a_subgraph_are_refused_before_one_exists(views, view):
    """``edge_weight`` with any mask and dropout with node masks: ``_resolve`` refuses them, so no subgraph of two kinds is ever built
    and the weighted sum takes none at all."""
    adj, X = views[view], torch.ones(N, 8)
    for family in FAMILIES:
        with pytest.raises(ValueError, match="row_mask / nbr_mask cannot be combined with edge_drop: not built"):
            _resolved(adj, family, "one", dict(edge_drop=(0.25, 7), row_mask=ROW_MASK))
    for kind in KINDS[1:]:
        with pytest.raises(ValueError, match="cannot be combined with .*: not built"):
            tiled.tiledMMFloat(adj, X, edge_weight=torch.zeros(0), **_keywords(kind, adj))
    assert "sub" not in inspect.signature(tiled._weighted).parameters


def test_every_declared_entry_of_the_families_is_named_by_a_route(views):
    want = {name for name in _declared(cabi.ATTN_HEADS_HEADER, cabi.FANOUT_HEADER, cabi.BLOCKS_HEADER)
            if name.startswith(("qgtc_tiledmm_f32", "qgtc_tiledmax_f32", "qgtc_tiledatt_", "qgtc_rowdot_"))}
    named = set()
    for family, heads, view, kind in CROSS:
        adj = views[view]
        try:
            H, (_, sub, _) = _resolved(adj, family, heads, _keywords(kind, adj))
        except ValueError:
            continue
        how, names = _route(family, H, adj.transposed, sub)
        if how == "entry":
            named.add(names)
    assert tiled._c_route(2, tiled._ALL) and not tiled._c_route(0, tiled._ALL)   # the row dot: heads through its C entry
    named.add(tiled._c_name("qgtc_rowdot_f32", 2, False))
    unreachable = {}   # name -> reason, for a declared entry no public call reaches; none today
    assert want - named == set(unreachable), sorted(want - named)
    assert named <= want | _declared(cabi.HEADER), sorted(named - want)


def test_the_other_view_of_every_kind(views):
    adj, t = views["row"], views["column"]
    for kind in KINDS:
        for view in (adj, t):
            _, (_, sub, _) = _resolved(view, "sum", "one", _keywords(kind, adj))
            assert sub.other().other() == sub, kind
            assert (sub.other() is sub) == (kind != "node masks")
            assert sub.rebuilt(sub.tensors()) == sub or "sample" in kind
    masks = tiled._Subgraph.of(row_mask=ROW_MASK, nbr_mask=NBR_MASK)
    assert masks.other() == tiled._Subgraph.of(row_mask=NBR_MASK, nbr_mask=ROW_MASK)
    assert masks.c_tail(adj) == (ROW_MASK.data_ptr(), NBR_MASK.data_ptr(), WORDS) and masks.suffix == "_nodes"
    assert tiled._Subgraph.of(key=(1 << 30, 7)).c_tail(t) == (1 << 30, 7) and tiled._ALL.c_tail(adj) == ()
    # a masked sample taken on adj: own masks and thr_of_nbr = 0 on adj, the masks swapped and thr_of_nbr = 1 on adj.T
    sample = _keywords("masked sample", adj)["fanout"]
    sub = tiled._Subgraph.of(sample=sample)
    assert sub.c_tail(adj) == (sample.thr.data_ptr(), 0, 1, ROW_MASK.data_ptr(), NBR_MASK.data_ptr(), WORDS)
    assert sub.other().c_tail(t) == (sample.thr.data_ptr(), 1, 1, NBR_MASK.data_ptr(), ROW_MASK.data_ptr(), WORDS)
    assert tiled._Subgraph.of(sample=_keywords("sample", t)["fanout"]).c_tail(adj)[1:] == (1, 1)
    # rebuilt from the saved tensors: the same sample, on fresh FanoutSample
    again = sub.rebuilt(sub.tensors())
    assert again.sample is not sample and vars(again.sample) == vars(sample)
