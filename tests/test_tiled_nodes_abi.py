"""C-ABI and Python refusals of node masks (include/qgtc.h, "Node masks": qgtc_node_bitmap, qgtc_tiled_inv_degree and the eight _nodes
entries): the symbols are exported, the ABI version stays 11, every _nodes entry refuses what its _drop twin refuses, in its order, then
a short or misaligned mask, all before any device work; and the Python layer refuses bad masks on an adjacency of CPU tensors (no GPU
needed). The signatures come from the header (cabi.load())."""
import os

import pytest

from test_tiled_drop_abi import EALIGN, EINVAL, ESIZE, _buf, _common_refusals

ENTRIES = ("qgtc_tiledmm_f32_nodes", "qgtc_tiledmm_f32_t_nodes", "qgtc_tiledmax_f32_nodes", "qgtc_tiledmax_f32_t_nodes",
           "qgtc_tiledatt_f32_nodes", "qgtc_tiledatt_f32_t_nodes", "qgtc_tiledatt_grad_f32_nodes", "qgtc_tiledatt_grad_f32_t_nodes")
NAMES = ("qgtc_node_bitmap", "qgtc_tiled_inv_degree") + ENTRIES


@pytest.fixture(scope="module")
def lib():
    from qgtc_ppopp22_amd import cabi

    return cabi.load()


def test_symbols_and_version(lib):
    for name in NAMES:
        assert getattr(lib, name), name
    assert len(NAMES) == 10
    assert lib.qgtc_abi_version() == 11


def test_the_header_declares_the_entries():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qgtc.h")).read()
    assert "Node masks" in text
    for name in NAMES:
        assert f"int {name}(" in text, name
    assert "#define QGTC_ABI_VERSION 11" in text
    for name in ENTRIES:   # the masks sit where the _drop twin has `threshold, seed`
        decl = text[text.index(f"int {name}("):]
        decl = " ".join(decl[: decl.index(";")].split())
        assert decl.endswith("const uint32_t *row_mask, const uint32_t *nbr_mask, size_t mask_words, void *stream)"), name
        twin = text[text.index(f"int {name[:-6]}_drop("):]
        twin = " ".join(twin[: twin.index(";")].split())
        assert decl.replace("_nodes(", "_drop(").replace("const uint32_t *row_mask, const uint32_t *nbr_mask, size_t mask_words",
                                                         "uint32_t threshold, uint64_t seed") == twin, name


def test_node_bitmap_and_inv_degree_refuse_bad_arguments(lib):
    keep, p = _buf(1 << 12)
    assert lib.qgtc_node_bitmap(None, 100, p, 4, None) == EINVAL
    assert lib.qgtc_node_bitmap(p, 100, None, 4, None) == EINVAL
    for n in (0, -1, (1 << 23) + 1):
        assert lib.qgtc_node_bitmap(p, n, p, 1 << 12, None) == EINVAL
    for off in (4, 8, 12, 1):
        assert lib.qgtc_node_bitmap(p, 100, p + off, 4, None) == EALIGN
    assert lib.qgtc_node_bitmap(p, 100, p, 3, None) == ESIZE          # S128(100) * 4 = 4
    assert lib.qgtc_node_bitmap(p, 129, p, 7, None) == ESIZE          # S128(129) * 4 = 8
    assert lib.qgtc_node_bitmap(p, 0, p + 4, 0, None) == EINVAL       # invalid beats misaligned
    assert lib.qgtc_node_bitmap(p, 100, p + 4, 3, None) == EALIGN     # misaligned beats short
    assert lib.qgtc_node_bitmap(p + 1, 100, p, 3, None) == ESIZE      # the flags are bytes: any address
    assert lib.qgtc_tiled_inv_degree(None, 10, p, None) == EINVAL
    assert lib.qgtc_tiled_inv_degree(p, 10, None, None) == EINVAL
    for n in (0, -1, (1 << 23) + 1):
        assert lib.qgtc_tiled_inv_degree(p, n, p, None) == EINVAL
    for off in (1, 2, 3):
        assert lib.qgtc_tiled_inv_degree(p + off, 10, p, None) == EALIGN
        assert lib.qgtc_tiled_inv_degree(p, 10, p + off, None) == EALIGN


def _mask_refusals(fn, ok, none, p):
    """what the masks add, after the twin's refusals: QGTC_ESIZE for mask_words < S128(n) * 4 when a mask is given, QGTC_EALIGN for a
    mask off a 16-byte boundary; either mask alone is checked the same way"""
    for idx, T in ((ok, 1), (none, 0)):
        for mask in ((p, p, 3), (p, None, 3), (None, p, 3), (p, p, 0)):
            assert fn(idx, T, 100, 8, mask=mask) == ESIZE, mask            # S128(100) * 4 = 4
        assert fn(idx, T, 129, 8, x_elems=1 << 16, out_elems=1 << 16, mask=(p, p, 7)) == ESIZE      # S128(129) * 4 = 8
        for off in (4, 8, 12, 1, 2):
            assert fn(idx, T, 100, 8, mask=(p + off, p, 4)) == EALIGN, off
            assert fn(idx, T, 100, 8, mask=(p, p + off, 4)) == EALIGN, off
            assert fn(idx, T, 100, 8, mask=(p + off, None, 4)) == EALIGN, off
            assert fn(idx, T, 100, 8, mask=(None, p + off, 4)) == EALIGN, off
        assert fn(idx, T, 100, 8, mask=(p + 4, p, 3)) == ESIZE             # short beats misaligned
    # the twin's refusals come first, and no mask lifts one
    for mask in ((None, None, 0), (p, p, 4), (p + 4, p, 3)):
        assert fn(ok, 1, 0, 8, mask=mask) == EINVAL
        assert fn(ok, 1, 100, 8, x_elems=799, mask=mask) == ESIZE
        assert fn(ok, 1, 100, 8, X=p + 1, mask=mask) == EALIGN


@pytest.mark.parametrize("transposed", [False, True])
def test_float_nodes_entries_refuse_bad_arguments(lib, transposed):
    keep, p = _buf(1 << 16)
    big = 1 << 16
    entry = lib.qgtc_tiledmm_f32_t_nodes if transposed else lib.qgtc_tiledmm_f32_nodes

    def fn(idx, T, n, N, x_elems=big, out_elems=big, X=p, out=p, row_scale=None, src_scale=None, mask=(p, p, big)):
        return entry(*idx, T, n, X, x_elems, N, row_scale, src_scale, out, out_elems, *mask, None)

    ok = (p,) * (4 if transposed else 3)
    none = (None,) * len(ok)
    _common_refusals(fn, ok, none, 799)
    for name in ("row_scale", "src_scale"):                   # both scales are optional, and aligned when given
        for off in (1, 2, 3):
            assert fn(ok, 1, 100, 8, **{name: p + off}) == EALIGN, name
        assert fn(ok, 1, 100, 8, x_elems=799, **{name: p}) == ESIZE
        assert fn(ok, 1, 0, 8, **{name: p + 1}) == EINVAL
    _mask_refusals(fn, ok, none, p)


@pytest.mark.parametrize("transposed", [False, True])
def test_max_nodes_entries_refuse_bad_arguments(lib, transposed):
    keep, p = _buf(1 << 16)
    big = 1 << 16
    entry = lib.qgtc_tiledmax_f32_t_nodes if transposed else lib.qgtc_tiledmax_f32_nodes

    def fn(idx, T, n, N, x_elems=big, out_elems=big, X=p, out=p, op=0, arg=None, arg_elems=0, mask=(p, p, big)):
        return entry(*idx, T, n, X, x_elems, N, op, out, out_elems, arg, arg_elems, *mask, None)

    ok = (p,) * (4 if transposed else 3)
    none = (None,) * len(ok)
    _common_refusals(fn, ok, none, 799)
    for op in (-1, 2, 9):
        assert fn(ok, 1, 100, 8, op=op) == EINVAL
    for op in (0, 1):
        for off in (1, 2, 3):
            assert fn(ok, 1, 100, 8, op=op, arg=p + off, arg_elems=big) == EALIGN
        assert fn(ok, 1, 100, 8, op=op, arg=p, arg_elems=799) == ESIZE
    _mask_refusals(fn, ok, none, p)


@pytest.mark.parametrize("grad", [False, True])
@pytest.mark.parametrize("transposed", [False, True])
def test_attention_nodes_entries_refuse_bad_arguments(lib, transposed, grad):
    keep, p = _buf(1 << 16)
    big = 1 << 16
    entry = getattr(lib, ("qgtc_tiledatt_grad_f32" if grad else "qgtc_tiledatt_f32") + ("_t" if transposed else "") + "_nodes")
    vectors = ("own", "nbr", "m", "inv", "D") if grad else ("own", "nbr", "shift", "m", "inv")

    def fn(idx, T, n, N, x_elems=big, out_elems=big, X=p, out=p, other=p, slope=0.2, flag=0, mask=(p, p, big), **vec):
        v = {name: vec.pop(name, p) for name in vectors}
        assert not vec, vec
        if grad:
            return entry(*idx, T, n, X, other, x_elems, N, v["own"], v["nbr"], slope, flag, v["m"], v["inv"], v["D"], out, out_elems,
                         *mask, None)
        return entry(*idx, T, n, X, x_elems, N, v["own"], v["nbr"], slope, flag, v["shift"], v["m"], v["inv"], out, out_elems, *mask, None)

    ok = (p,) * (4 if transposed else 3)
    none = (None,) * len(ok)
    _common_refusals(fn, ok, none, 99 if grad else 799)
    for slope in (-0.001, 1.001, float("nan")):
        assert fn(ok, 1, 100, 8, slope=slope) == EINVAL
    for flag in (-1, 2):
        assert fn(ok, 1, 100, 8, flag=flag) == EINVAL
    for name in vectors:
        assert fn(ok, 1, 100, 8, **{name: None}) == EINVAL, name
        assert fn(ok, 1, 100, 8, **{name: p + 2}) == EALIGN, name
    _mask_refusals(fn, ok, none, p)


# ---- the Python layer, on an adjacency of CPU tensors: every refusal comes before the binding is reached ------------------------------------
@pytest.fixture(scope="module")
def cpu_adj():
    import torch

    from qgtc_ppopp22_amd.tiled import TiledAdjacency

    n = 200
    return TiledAdjacency(n, torch.zeros((n + 31) // 32 + 1, dtype=torch.int64), torch.zeros(0, dtype=torch.int32),
                          torch.zeros((0, 32, 4), dtype=torch.int32))


def test_python_refuses_bad_masks(cpu_adj):
    import torch

    import QGTC

    n, words = cpu_adj.n, 8
    X = torch.zeros(n, 4)
    good = torch.zeros(words, dtype=torch.int32)
    p = torch.zeros(n)
    modes = ({}, {"reduce": "max"}, {"attn": (p, p)})
    for call in (QGTC.tiledMMFloat, QGTC.tiledAggregate):
        for mode in modes:
            for name in ("row_mask", "nbr_mask"):
                for bad in (good.to(torch.int64), good.to(torch.float32), good.to(torch.bool), good.view(torch.uint8), [0] * words, 7):
                    with pytest.raises(TypeError, match=name):
                        call(cpu_adj, X, **mode, **{name: bad})
                for bad in (torch.zeros(words - 4, dtype=torch.int32), torch.zeros(words + 4, dtype=torch.int32),
                            torch.zeros((2, 4), dtype=torch.int32), torch.zeros(2 * words, dtype=torch.int32)[::2],
                            torch.zeros(words, dtype=torch.int32, device="meta")):
                    with pytest.raises(ValueError, match=name):
                        call(cpu_adj, X, **mode, **{name: bad})
                with pytest.raises(ValueError, match="edge_drop"):
                    call(cpu_adj, X, **mode, edge_drop=(0.5, 1), **{name: good})
    for method in (cpu_adj.degrees, cpu_adj.mean_scale, cpu_adj.sym_scale):
        with pytest.raises(TypeError, match="row_mask"):
            method(row_mask=good.to(torch.int64))
        with pytest.raises(ValueError, match="nbr_mask"):
            method(nbr_mask=torch.zeros(4, dtype=torch.int32))


def test_node_bitmap_refuses_bad_nodes():
    import torch

    from qgtc_ppopp22_amd.tiled import node_bitmap

    with pytest.raises(TypeError):
        node_bitmap([0, 1], 10)
    for bad in (torch.zeros(10, dtype=torch.int32), torch.zeros(10), torch.zeros(10, dtype=torch.uint8)):
        with pytest.raises(TypeError, match="bool or int64"):
            node_bitmap(bad, 10)
    for bad in (torch.zeros(9, dtype=torch.bool), torch.zeros(11, dtype=torch.bool), torch.zeros((10, 1), dtype=torch.bool)):
        with pytest.raises(ValueError, match="shape"):
            node_bitmap(bad, 10)
    for bad in (torch.tensor([0, 10]), torch.tensor([-1]), torch.tensor([3, 3, 2 ** 40])):
        with pytest.raises(ValueError, match="outside"):
            node_bitmap(bad, 10)
    with pytest.raises(ValueError, match="one dimension"):
        node_bitmap(torch.zeros((2, 2), dtype=torch.int64), 10)
    for n in (0, -3, (1 << 23) + 1):
        with pytest.raises(ValueError, match="n must"):
            node_bitmap(torch.zeros(max(n, 0), dtype=torch.bool), n)


def test_layers_refuse_nodes_where_it_is_not_built(cpu_adj):
    import torch

    from qgtc_ppopp22_amd import conv

    n = cpu_adj.n
    X, nodes = torch.zeros(n, 4), torch.ones(n, dtype=torch.bool)
    layer = conv.GCNConv(4, 4, 4)
    with pytest.raises(NotImplementedError, match="dense"):
        layer(torch.eye(n), X, nodes=nodes)
    for make in (lambda: conv.GCNConv(4, 4, 4, edge_drop=0.5), lambda: conv.GATConv(4, 4, edge_drop=0.5)):
        with pytest.raises(NotImplementedError, match="edge_drop"):
            make()(cpu_adj, X, edge_seed=1, nodes=nodes)
    for layer in (conv.GCNConv(4, 4, 4), conv.GATConv(4, 4)):
        with pytest.raises(TypeError, match="bool"):
            layer(cpu_adj, X, nodes=torch.arange(n))
        with pytest.raises(ValueError, match="shape"):
            layer(cpu_adj, X, nodes=torch.ones(n - 1, dtype=torch.bool))
