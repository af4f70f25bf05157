"""C-ABI of the source-scaled float tiled products and the inverse square roots of the degrees (include/qgtc.h, "Source scale":
qgtc_tiledmm_f32_src / qgtc_tiledmm_f32_t_src / qgtc_tiled_inv_sqrt_degree): the symbols are exported, the ABI version stays 11, bad
arguments are refused before any device work, and the Python layer (QGTC.tiledMMFloat(src_scale=), QGTC.tiledAggregate) refuses what
it must before it reaches the extension (no GPU needed). The signatures come from the header (cabi.load())."""
import ctypes

import pytest

OK, EINVAL, ESIZE, EALIGN = 0, 1, 2, 3


@pytest.fixture(scope="module")
def lib():
    from qgtc_ppopp22_amd import cabi

    return cabi.load()


def _buf(words):
    b = (ctypes.c_uint32 * (words + 64))()
    addr = ctypes.addressof(b)
    return b, (addr + 255) & ~255   # keep the buffer alive; 256-byte aligned address inside it


def test_symbols_and_version(lib):
    assert lib.qgtc_tiledmm_f32_src and lib.qgtc_tiledmm_f32_t_src and lib.qgtc_tiled_inv_sqrt_degree
    assert lib.qgtc_tiledmm_f32 and lib.qgtc_tiledmm_f32_t      # the entries they extend are still there
    assert lib.qgtc_abi_version() == 11


@pytest.mark.parametrize("with_src", [True, False], ids=["src_scale", "src_scale NULL"])
@pytest.mark.parametrize("transposed", [False, True])
def test_source_scaled_products_refuse_bad_arguments(lib, transposed, with_src):
    """Every refusal of qgtc_tiledmm_f32 / _t, with a source scale and with NULL in its place (the call is then the parent entry's)."""
    keep, p = _buf(1 << 16)
    big = 1 << 16
    entry = lib.qgtc_tiledmm_f32_t_src if transposed else lib.qgtc_tiledmm_f32_src
    src = p if with_src else None

    def fn(idx, T, n, N, x_elems=big, out_elems=big, X=p, scale=p, src_scale=src, out=p):
        """idx: the index pointers and the tile words (3 forward: row_ptr, kquad, tiles; 4 transposed: col_ptr, col_tile, col_rb, tiles)"""
        return entry(*idx, T, n, X, x_elems, N, scale, src_scale, out, out_elems, None)

    ok = (p,) * (4 if transposed else 3)
    assert fn(ok, 1, 0, 8) == EINVAL                          # n < 1
    assert fn(ok, 1, -5, 8) == EINVAL
    assert fn(ok, 1, (1 << 23) + 1, 8) == EINVAL              # n > 2^23
    assert fn(ok, 1, 100, 0) == EINVAL                        # N < 1
    assert fn(ok, 1, 100, -3) == EINVAL
    assert fn(ok, -1, 100, 8) == EINVAL                       # negative n_tiles
    for k in range(len(ok)):                                  # tiles without row_ptr / kquad / col_ptr / col_tile / col_rb / tile words
        assert fn(ok[:k] + (None,) + ok[k + 1:], 1, 100, 8) == EINVAL, k
    assert fn(ok, 1, 100, 8, X=None) == EINVAL                # no X
    assert fn(ok, 1, 100, 8, out=None) == EINVAL              # no out
    assert fn((None,) * len(ok), 0, 100, 8, X=None) == EINVAL     # ... also without tiles
    assert fn((None,) * len(ok), 0, 100, 8, out=None) == EINVAL
    assert fn(ok, 1, 100, 8, x_elems=799) == ESIZE            # one float short of 100 x 8
    assert fn(ok, 1, 100, 8, out_elems=799) == ESIZE
    assert fn(ok, 1, 100, 8, scale=None, out_elems=799) == ESIZE
    assert fn(ok, 1, 1 << 23, 1 << 20, x_elems=(1 << 43) - 1, out_elems=1 << 43) == ESIZE   # n * N does not wrap in 32 bits
    assert fn(ok[:-1] + (p + 4,), 1, 100, 8) == EALIGN        # tiles off a 16-byte boundary
    assert fn(ok[:-1] + (p + 8,), 1, 100, 8) == EALIGN
    for off in (1, 2, 3):
        assert fn(ok, 1, 100, 8, X=p + off) == EALIGN         # X off a 4-byte boundary
        assert fn(ok, 1, 100, 8, out=p + off) == EALIGN       # out off a 4-byte boundary
        assert fn(ok, 1, 100, 8, scale=p + off) == EALIGN     # row_scale off a 4-byte boundary
        assert fn(ok, 1, 100, 8, src_scale=p + off) == EALIGN          # src_scale off a 4-byte boundary
        assert fn(ok, 1, 100, 8, scale=None, src_scale=p + off) == EALIGN
        assert fn(ok, 1, 100, 8, src_scale=p + off, out_elems=799) == EALIGN    # alignment is checked before the sizes, as for the others
        assert fn(ok, 1, 0, 8, src_scale=p + off) == EINVAL            # and the domain before the alignment


def test_inverse_square_roots_refuse_bad_arguments(lib):
    keep, p = _buf(1 << 10)
    fn = lib.qgtc_tiled_inv_sqrt_degree
    assert fn(None, 100, p, None) == EINVAL
    assert fn(p, 100, None, None) == EINVAL
    assert fn(p, 0, p, None) == EINVAL
    assert fn(p, -1, p, None) == EINVAL
    assert fn(p, (1 << 23) + 1, p, None) == EINVAL
    for off in (1, 2, 3):
        assert fn(p + off, 100, p, None) == EALIGN
        assert fn(p, 100, p + off, None) == EALIGN


# ---- the Python layer: refusals made before the extension is called, on an adjacency of CPU tensors ----------------------------------------
@pytest.fixture(scope="module")
def cpu_adj():
    import torch

    from qgtc_ppopp22_amd.tiled import TiledAdjacency

    n = 40
    adj = TiledAdjacency(n, torch.zeros((n + 31) // 32 + 1, dtype=torch.int64), torch.zeros(0, dtype=torch.int32),
                         torch.zeros((0, 32, 4), dtype=torch.int32))
    return adj


@pytest.mark.parametrize("fn_name", ["tiledMMFloat", "tiledAggregate"])
def test_python_refusals_name_src_scale(cpu_adj, fn_name):
    import numpy as np
    import torch

    import qgtc_ppopp22_amd.tiled as tiled

    fn = getattr(tiled, fn_name)
    n, N = cpu_adj.n, 8
    X = torch.ones(n, N)
    good = torch.ones(n)
    bad = [(TypeError, "src_scale must be float32", good.double()),
           (TypeError, "src_scale must be float32", good.to(torch.int32)),
           (TypeError, "src_scale must be a torch.Tensor", np.ones(n, np.float32)),
           (ValueError, rf"src_scale must have shape \[{n}\]", torch.ones(n + 1)),
           (ValueError, rf"src_scale must have shape \[{n}\]", torch.ones(n, 1)),
           (ValueError, "src_scale must be on the adjacency's device", torch.ones(n, device="meta")),
           (ValueError, "src_scale must be contiguous", torch.ones(2 * n)[::2])]
    for exc, match, sc in bad:
        with pytest.raises(exc, match=match):
            fn(cpu_adj, X, None, sc)
        with pytest.raises(exc, match=match):
            fn(cpu_adj, X, good, src_scale=sc)
    with pytest.raises(TypeError, match="row_scale must be float32"):      # the row scale's messages keep its name
        fn(cpu_adj, X, good.double(), good)
    with pytest.raises(TypeError, match="X must be float32"):
        fn(cpu_adj, X.double(), None, good)


def test_a_scale_that_requires_grad_is_refused(cpu_adj):
    import torch

    import qgtc_ppopp22_amd.tiled as tiled

    n = cpu_adj.n
    X = torch.ones(n, 8, requires_grad=True)
    with pytest.raises(ValueError, match="row_scale must not require a gradient"):
        tiled.tiledAggregate(cpu_adj, X, torch.ones(n, requires_grad=True), None)
    with pytest.raises(ValueError, match="src_scale must not require a gradient"):
        tiled.tiledAggregate(cpu_adj, X, torch.ones(n), torch.ones(n, requires_grad=True))


def test_the_public_names():
    import QGTC
    import qgtc_ppopp22_amd.tiled as tiled

    for name in ("tiledAggregate", "add_self_loops", "tiledMMFloat"):
        assert name in tiled.__all__ and getattr(QGTC, name) is getattr(tiled, name)
    assert hasattr(tiled.TiledAdjacency, "sym_scale")
    from qgtc_ppopp22_amd.conv import GCNConv

    assert GCNConv(4, 4, 2).norm is None and GCNConv(4, 4, 2, norm="sym").norm == "sym"
    with pytest.raises(ValueError, match="norm"):
        GCNConv(4, 4, 2, norm="max")
    import torch

    with pytest.raises(NotImplementedError, match="pack_edges_tiled"):
        GCNConv(4, 4, 2, norm="mean")(torch.zeros(3, 3), torch.zeros(3, 4))
    m = GCNConv(4, 4, 2)
    A, X = torch.rand(3, 3), torch.rand(3, 4)
    assert torch.equal(m(A, X), torch.mm(A, torch.mm(torch.mm(A, torch.mm(X, m.W_in)), m.W_out)))   # dense, norm=None: what it was
