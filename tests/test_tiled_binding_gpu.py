"""The refusals of the tiled bindings themselves (qgtc_torch.cpp: _tiled_mm, _tiled_mm_t, _tiled_mm_f32, _tiled_mm_f32_t, _tiled_mm_f32_src,
_tiled_mm_f32_t_src, _tiled_degrees, _tiled_colindex), called past the Python layer that normally checks first: a malformed view of the
adjacency, an operand on the host, and the mask combinations that are not built are each a RuntimeError. Every input here is stopped by
a host check of the binding BEFORE anything is launched: no case hands a kernel inconsistent pointers, and none may be added that would.

The graph is a 40-node ring with three chords: two 32-row blocks and one k-quad, the smallest adjacency whose row_ptr (3 entries) and
col_ptr (2 entries) differ in length, so a view handed the other view's pointer array is refused by its length alone."""
import pytest

pytestmark = pytest.mark.gpu

N_NODES, N_FEATS, BIT2 = 40, 8, 2
ROW_VIEW, COL_VIEW = ("row_ptr", "kquad"), ("col_ptr", "col_tile", "col_rb")


@pytest.fixture(scope="module")
def graph(qgtc):
    """The adjacency, its operands and, per binding, the keyword arguments of a call that is fine."""
    import types

    import torch

    from qgtc_ppopp22_amd.tiled import _ext, _value_index

    n, N = N_NODES, N_FEATS
    ring = torch.arange(n)
    src = torch.cat([ring, torch.tensor([0, 5, 12])]).cuda()
    dst = torch.cat([(ring + 1) % n, torch.tensor([20, 33, 3])]).cuda()
    adj = qgtc.pack_edges_tiled(src, dst, n)
    t = adj.T
    assert adj.n_tiles == 2 and adj.row_ptr.numel() == 3 and t.col_ptr.numel() == 2
    X = torch.arange(n * N, dtype=torch.float32, device="cuda").reshape(n, N) % 3
    bit_X = qgtc.val2bit(X, BIT2, True, False)
    row = dict(row_ptr=adj.row_ptr, kquad=adj.kquad, tiles=adj.tiles, n=n)
    col = dict(col_ptr=t.col_ptr, col_tile=t.col_tile, col_rb=t.col_rb, tiles=adj.tiles, n=n)
    bits = dict(bit_X=bit_X, N=N, bit2=BIT2, output_bit=BIT2, to_float=True)
    scale = torch.ones(n, device="cuda")
    good = {"_tiled_mm": {**row, **bits}, "_tiled_mm_t": {**col, **bits},
            "_tiled_mm_f32": {**row, "X": X}, "_tiled_mm_f32_t": {**col, "X": X},
            "_tiled_mm_f32_src": {**row, "X": X, "row_scale": None, "src_scale": scale},
            "_tiled_mm_f32_t_src": {**col, "X": X, "row_scale": None, "src_scale": scale},
            "_tiled_degrees": dict(row), "_tiled_colindex": dict(row_ptr=adj.row_ptr, kquad=adj.kquad, n=n)}
    val_ptr, val_row, nnz = _value_index(adj)
    return types.SimpleNamespace(torch=torch, ext=_ext, adj=adj, X=X, good=good, row=row, col=col, scale=scale,
                                 mask=torch.full(((n + 127) // 128 * 4,), -1, dtype=torch.int32, device="cuda"),
                                 edge_values=(val_ptr, val_row, torch.ones(nnz, device="cuda")))


BINDINGS = ("_tiled_mm", "_tiled_mm_t", "_tiled_mm_f32", "_tiled_mm_f32_t", "_tiled_mm_f32_src", "_tiled_mm_f32_t_src", "_tiled_degrees",
            "_tiled_colindex")


@pytest.mark.parametrize("name", BINDINGS)
def test_a_malformed_view_or_operand_is_refused(graph, name):
    torch, fn, good = graph.torch, getattr(graph.ext, name), graph.good[name]
    wrong = {torch.int64: torch.int32, torch.int32: torch.int64}
    faults = []
    for key in ROW_VIEW + COL_VIEW:                                # an index tensor of the wrong dtype
        if key in good:
            faults.append(({key: good[key].to(wrong[good[key].dtype])}, "int64"))
    ptr = "row_ptr" if "row_ptr" in good else "col_ptr"
    faults.append(({ptr: good[ptr][:-1].contiguous()}, "entries"))  # row_ptr / col_ptr one element short
    if "tiles" in good:
        faults.append(({"tiles": good["tiles"][:-1].contiguous()}, "tiles"))   # a tile's worth of words missing
    faults.append(({"n": 0}, "n must lie in"))
    for key in ("X", "bit_X"):                                     # the operand on the host
        if key in good:
            faults.append(({key: good[key].cpu()}, "must be a CUDA tensor"))
    assert len(faults) >= 4
    for change, match in faults:
        with pytest.raises(RuntimeError, match=match):
            fn(**{**good, **change})


@pytest.mark.parametrize("view", ["row", "col"])
def test_mask_combinations_that_are_not_built_are_refused(graph, view):
    torch, X = graph.torch, graph.X
    fn = graph.ext._tiled_mm_f32 if view == "row" else graph.ext._tiled_mm_f32_t
    src_fn = graph.ext._tiled_mm_f32_src if view == "row" else graph.ext._tiled_mm_f32_t_src
    idx = getattr(graph, view)
    drop, nodes = dict(edge_drop=(1 << 31, 3)), dict(node_masks=(graph.mask, graph.mask))
    s = graph.scale
    att = dict(att_own=s, att_nbr=s, shift=s)
    both = "node_masks cannot be combined with edge_drop"
    with pytest.raises(RuntimeError, match=both):
        fn(**idx, X=X, **drop, **nodes)
    with pytest.raises(RuntimeError, match=both):
        src_fn(**idx, X=X, row_scale=None, src_scale=s, **drop, **nodes)
    for reduce in ("max", "min"):
        with pytest.raises(RuntimeError, match=both):
            fn(**idx, X=X, reduce=reduce, **drop, **nodes)
    with pytest.raises(RuntimeError, match=both):
        fn(**idx, X=X, att_mode="forward", **att, **drop, **nodes)
    arg = torch.zeros(N_NODES, N_FEATS, dtype=torch.int32, device="cuda")
    for mask, word in ((drop, "edge_drop"), (nodes, "node_masks")):
        with pytest.raises(RuntimeError, match=f'reduce="select" takes no {word}'):
            fn(**idx, X=X, reduce="select", arg=arg, **mask)
        with pytest.raises(RuntimeError, match='att_mode="rowdot" takes no edge_drop or node_masks'):
            fn(**idx, X=X, att_mode="rowdot", other=X, **mask)
        with pytest.raises(RuntimeError, match="edge_values cannot be combined with edge_drop or node_masks"):
            fn(**idx, X=X, edge_values=graph.edge_values, **mask)
