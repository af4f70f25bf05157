"""C-ABI of fixed-fanout sampling (include/qgtc_fanout.h: the two selection entries and the _fanout twins of the eight _drop entries): the
header parses with cabi.signatures(text) to the ten entries, every entry is exported and bound by cabi.load(), the header's own golden
file holds, the four earlier headers, their golden files and ABI version 11 are untouched, bad arguments are refused before any device
work in the project's order - invalid, then misaligned, then short -, and ``fanout=`` of the Python layer refuses what is not built (no
GPU needed)."""
import ctypes
import os

import pytest

from qgtc_ppopp22_amd import cabi
from test_cabi import _lines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, ESIZE, EALIGN = 0, 1, 2, 3
SELECT = ("qgtc_tiled_fanout_thr", "qgtc_tiled_fanout_thr_t")
TWINS = ("qgtc_tiledmm_f32", "qgtc_tiledmm_f32_t", "qgtc_tiledmax_f32", "qgtc_tiledmax_f32_t", "qgtc_tiledatt_f32", "qgtc_tiledatt_f32_t",
         "qgtc_tiledatt_grad_f32", "qgtc_tiledatt_grad_f32_t")
ENTRIES = SELECT + tuple(t + "_fanout" for t in TWINS)
V, I, Z, F, P64, U64, U32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_float, ctypes.c_int64, ctypes.c_uint64, ctypes.c_uint32


def fanout_signatures():
    with open(cabi.FANOUT_HEADER) as f:
        return cabi.signatures(f.read())


@pytest.fixture(scope="module")
def lib():
    return cabi.load()


@pytest.fixture(scope="module")
def p():
    b = (ctypes.c_uint32 * ((1 << 16) + 64))()
    addr = (ctypes.addressof(b) + 255) & ~255   # 256-byte aligned address inside the buffer
    yield addr
    del b


def test_the_header_parses_to_the_ten_entries():
    sig = fanout_signatures()
    assert list(sig) == list(ENTRIES) and len(sig) == 10
    assert sig[SELECT[0]] == (I, [V, V, V, P64, I, I, U64, V, Z, V])
    assert sig[SELECT[1]] == (I, [V, V, V, V, P64, I, I, U64, V, Z, V])
    # each twin is its _drop twin with (thr, thr_of_nbr, seed) in place of (threshold, seed)
    drop = cabi.signatures()
    for t in TWINS:
        ret, args = drop[t + "_drop"]
        assert args[-3:] == [U32, U64, V]
        assert sig[t + "_fanout"] == (ret, args[:-3] + [V, I, U64, V]), t


def test_the_golden_file_holds():
    golden = open(os.path.join(ROOT, "tests", "golden", "qgtc_fanout_abi.txt")).read().splitlines()
    assert _lines(fanout_signatures()) == golden and len(golden) == 10


def test_every_entry_is_exported_and_bound(lib):
    for name, (ret, args) in fanout_signatures().items():
        fn = getattr(lib, name)
        assert fn.restype is ret and list(fn.argtypes) == args, name


def test_the_earlier_headers_are_untouched(lib):
    sig = cabi.signatures()
    texts = {h: open(h).read() for h in (cabi.HEADER, cabi.HEADS_HEADER, cabi.ATTN_HEADS_HEADER, cabi.ADDSCORE_HEADER)}
    for text in texts.values():
        assert not set(cabi.signatures(text)) & set(ENTRIES) and "fanout" not in text
    assert lib.qgtc_abi_version() == 11
    assert "#define QGTC_ABI_VERSION 11" in texts[cabi.HEADER]
    golden = os.path.join(ROOT, "tests", "golden")
    assert _lines(sig) == open(os.path.join(golden, "qgtc_abi.txt")).read().splitlines()
    for header, name in ((cabi.HEADS_HEADER, "qgtc_heads_abi.txt"), (cabi.ATTN_HEADS_HEADER, "qgtc_attn_heads_abi.txt"),
                         (cabi.ADDSCORE_HEADER, "qgtc_addscore_abi.txt")):
        assert _lines(cabi.signatures(texts[header])) == open(os.path.join(golden, name)).read().splitlines()


@pytest.mark.parametrize("transposed", [False, True])
def test_the_selection_refuses_bad_arguments(lib, p, transposed):
    entry = lib.qgtc_tiled_fanout_thr_t if transposed else lib.qgtc_tiled_fanout_thr
    w = 4 if transposed else 3

    def f(idx=(p,) * w, T=2, n=100, k=3, seed=1, thr=p, te=100):
        return entry(*idx, T, n, k, seed, thr, te, None)

    assert f(n=0) == EINVAL and f(n=(1 << 23) + 1) == EINVAL and f(T=-1) == EINVAL
    assert f(k=0) == EINVAL and f(k=-1) == EINVAL and f(thr=None) == EINVAL
    for i in range(w):
        assert f(idx=tuple(None if j == i else p for j in range(w))) == EINVAL
    assert f(idx=(p,) * (w - 1) + (p + 4,)) == EALIGN and f(thr=p + 2) == EALIGN
    assert f(te=99) == ESIZE and f(te=0) == ESIZE
    # the order: invalid before misaligned before short
    assert f(thr=p + 2, k=0) == EINVAL and f(idx=(p,) * (w - 1) + (p + 4,), thr=None) == EINVAL
    assert f(te=99, thr=p + 2) == EALIGN and f(te=99, k=0) == EINVAL
    # an adjacency without tiles is still checked
    none = dict(idx=(None,) * w, T=0)
    assert f(**none, k=0) == EINVAL and f(**none, thr=None) == EINVAL and f(**none, thr=p + 2) == EALIGN and f(**none, te=99) == ESIZE


def _twin_call(lib, p, stem, transposed):
    """f(**overrides) for one twin on valid arguments, and the names of its pointer arguments that must not be NULL"""
    big = 1 << 16
    w = 4 if transposed else 3
    entry = getattr(lib, stem + ("_t" if transposed else "") + "_fanout")
    if stem == "qgtc_tiledmm_f32":
        def f(idx=(p,) * w, T=2, n=100, X=p, xe=big, N=8, rs=p, cs=p, out=p, oe=big, thr=p, nbr=0, seed=1):
            return entry(*idx, T, n, X, xe, N, rs, cs, out, oe, thr, nbr, seed, None)
        return f, ("X", "out"), ("X", "out", "rs", "cs"), ("xe", "oe")
    if stem == "qgtc_tiledmax_f32":
        def f(idx=(p,) * w, T=2, n=100, X=p, xe=big, N=8, op=0, out=p, oe=big, arg=p, ae=big, thr=p, nbr=0, seed=1):
            return entry(*idx, T, n, X, xe, N, op, out, oe, arg, ae, thr, nbr, seed, None)
        return f, ("X", "out"), ("X", "out", "arg"), ("xe", "oe", "ae")
    if stem == "qgtc_tiledatt_f32":
        def f(idx=(p,) * w, T=2, n=100, X=p, xe=big, N=8, ao=p, an=p, slope=0.2, bwd=0, shift=p, m=p, inv=p, out=p, oe=big, thr=p, nbr=0,
              seed=1):
            return entry(*idx, T, n, X, xe, N, ao, an, slope, bwd, shift, m, inv, out, oe, thr, nbr, seed, None)
        return f, ("X", "ao", "an", "shift", "m", "inv", "out"), ("X", "ao", "an", "shift", "m", "inv", "out"), ("xe", "oe")

    def f(idx=(p,) * w, T=2, n=100, A=p, B=p, abe=big, N=8, ao=p, an=p, slope=0.2, owns=0, m=p, inv=p, D=p, out=p, oe=big, thr=p, nbr=0,
          seed=1):
        return entry(*idx, T, n, A, B, abe, N, ao, an, slope, owns, m, inv, D, out, oe, thr, nbr, seed, None)
    return f, ("A", "B", "ao", "an", "m", "inv", "D", "out"), ("A", "B", "ao", "an", "m", "inv", "D", "out"), ("abe", "oe")


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("stem", ["qgtc_tiledmm_f32", "qgtc_tiledmax_f32", "qgtc_tiledatt_f32", "qgtc_tiledatt_grad_f32"])
def test_the_twins_refuse_bad_arguments(lib, p, stem, transposed):
    f, needed, floats, sizes = _twin_call(lib, p, stem, transposed)
    w = 4 if transposed else 3
    off16 = (p,) * (w - 1) + (p + 4,)
    # invalid: the _drop twin's list, then a NULL thr and a thr_of_nbr outside {0, 1}
    assert f(n=0) == EINVAL and f(n=(1 << 23) + 1) == EINVAL and f(N=0) == EINVAL and f(T=-1) == EINVAL
    for name in needed:
        assert f(**{name: None}) == EINVAL, name
    for i in range(w):
        assert f(idx=tuple(None if j == i else p for j in range(w))) == EINVAL
    assert f(thr=None) == EINVAL
    for bad in (-1, 2, 3, 1 << 30):
        assert f(nbr=bad) == EINVAL, bad
    if stem == "qgtc_tiledmax_f32":
        assert f(op=2) == EINVAL and f(op=-1) == EINVAL
    if stem in ("qgtc_tiledatt_f32", "qgtc_tiledatt_grad_f32"):
        assert f(slope=1.5) == EINVAL and f(slope=float("nan")) == EINVAL
    # misaligned
    assert f(idx=off16) == EALIGN and f(thr=p + 2) == EALIGN and f(thr=p + 1, nbr=1) == EALIGN
    for name in floats:
        assert f(**{name: p + 2}) == EALIGN, name
    # short, in elements
    for name in sizes:
        assert f(**{name: 99}) == ESIZE, name
    # the order: QGTC_EINVAL, the new causes included, before QGTC_EALIGN before QGTC_ESIZE
    first, size = floats[0], sizes[0]
    assert f(idx=off16, thr=None) == EINVAL and f(idx=off16, nbr=2) == EINVAL
    assert f(**{first: p + 2}, thr=None) == EINVAL and f(**{first: p + 2}, nbr=-1) == EINVAL
    assert f(**{size: 99}, thr=None) == EINVAL and f(**{size: 99}, nbr=2) == EINVAL
    assert f(thr=p + 2, N=0) == EINVAL and f(thr=p + 2, **{needed[0]: None}) == EINVAL
    assert f(**{size: 99}, thr=p + 2) == EALIGN and f(**{size: 99}, **{first: p + 2}) == EALIGN
    # both forms are in the domain: the next refusal is reached
    assert f(nbr=0, **{size: 99}) == ESIZE and f(nbr=1, **{size: 99}) == ESIZE
    # an adjacency without tiles is still checked
    none = dict(idx=(None,) * w, T=0)
    assert f(**none, thr=None) == EINVAL and f(**none, nbr=2) == EINVAL and f(**none, thr=p + 2) == EALIGN
    assert f(**none, **{size: 99}) == ESIZE


# ---- the Python layer: what fanout= refuses, before any device work ------------------------------------------------------------------------
class _Stub:
    """an object the checks accept as a tensor would never get this far: the refusals below are made before any operand is read"""


def _adjacency():
    import torch

    from qgtc_ppopp22_amd import tiled

    n = 40
    adj = tiled.TiledAdjacency(n, torch.zeros(3, dtype=torch.int64), torch.zeros(0, dtype=torch.int32),
                               torch.zeros((0, 32, 4), dtype=torch.int32))
    return tiled, adj, torch.zeros((n, 4), dtype=torch.float32)


def test_fanout_refuses_what_is_not_built():
    import torch

    from qgtc_ppopp22_amd import fanout as fo

    tiled, adj, X = _adjacency()
    n = adj.n
    calls = (lambda **kw: tiled.tiledMMFloat(adj, X, **kw), lambda **kw: tiled.tiledAggregate(adj, X, **kw))
    bitmap = torch.zeros((n + 127) // 128 * 4, dtype=torch.int32)
    for call in calls:
        with pytest.raises(ValueError, match="fanout cannot be combined with edge_drop: not built"):
            call(fanout=(3, 1), edge_drop=(0.5, 1))
        with pytest.raises(ValueError, match="fanout cannot be combined with row_mask / nbr_mask: not built"):
            call(fanout=(3, 1), row_mask=bitmap)
        with pytest.raises(ValueError, match="fanout cannot be combined with row_mask / nbr_mask: not built"):
            call(fanout=(3, 1), nbr_mask=bitmap)
        with pytest.raises(ValueError, match="fanout cannot be combined with edge_weight: not built"):
            call(fanout=(3, 1), edge_weight=torch.zeros(0, dtype=torch.float32))
        with pytest.raises(ValueError, match=r"fanout cannot be combined with \[n, H\] scores: not built"):
            call(fanout=(3, 1), attn=(torch.zeros((n, 2)), torch.zeros((n, 2))))
        for k in (0, -1, -(1 << 40)):
            with pytest.raises(ValueError, match="k must be at least 1"):
                call(fanout=(k, 1))
        for k in (2.0, "3", None, True, torch.tensor(3)):
            with pytest.raises(TypeError, match="k must be an int"):
                call(fanout=(k, 1))
        for seed in (-1, 1 << 64):
            with pytest.raises(ValueError, match="seed"):
                call(fanout=(3, seed))
        for seed in (1.0, None, True, "1"):
            with pytest.raises(TypeError, match="seed"):
                call(fanout=(3, seed))
        for bad in (3, (3,), (3, 1, 2), "ab", {3: 1}):
            with pytest.raises(TypeError, match="pair"):
                call(fanout=bad)
        # a sample of another adjacency
        _, other, _ = _adjacency()
        stranger = fo.FanoutSample(other, 3, 1, torch.zeros(n, dtype=torch.int32))
        with pytest.raises(ValueError, match="sample of another adjacency"):
            call(fanout=stranger)
        # a hand-built sample of this adjacency: the C entries take no length for thr, so its tensor is checked here
        good = torch.zeros(n, dtype=torch.int32)
        for bad, error, match in ((good.tolist(), TypeError, "torch.Tensor"), (good.to(torch.int64), TypeError, "int32"),
                                  (good.to(torch.float32), TypeError, "int32"), (good[:-1], ValueError, "shape"),
                                  (torch.zeros(n + 1, dtype=torch.int32), ValueError, "shape"),
                                  (good.view(n // 2, 2), ValueError, "shape"), (torch.zeros(0, dtype=torch.int32), ValueError, "shape"),
                                  (torch.zeros(2 * n, dtype=torch.int32)[::2], ValueError, "contiguous"),
                                  (good.to("meta"), ValueError, "device")):
            for view in (adj, adj._other if adj._other is not None else adj):
                with pytest.raises(error, match=match):
                    call(fanout=fo.FanoutSample(view, 3, 1, bad))
        with pytest.raises(ValueError, match="k must be at least 1"):
            call(fanout=fo.FanoutSample(adj, 0, 1, good))
        with pytest.raises(ValueError, match="seed"):
            call(fanout=fo.FanoutSample(adj, 3, -1, good))
        with pytest.raises(ValueError, match="sample of another adjacency"):
            call(fanout=fo.FanoutSample("adj", 3, 1, good))
    with pytest.raises(ValueError, match="k must be at least 1"):
        fo.sample_fanout(adj, 0, 1)
    with pytest.raises(TypeError, match="k must be an int"):
        fo.sample_fanout(adj, 1.5, 1)
    with pytest.raises(TypeError, match="TiledAdjacency"):
        fo.sample_fanout("adj", 3, 1)


def test_sageconv_refuses_bad_arguments():
    from qgtc_ppopp22_amd import sage

    with pytest.raises(ValueError, match="aggr"):
        sage.SAGEConv(4, 4, aggr="sum")
    for bad in (0, -3):
        with pytest.raises(ValueError, match="fanout"):
            sage.SAGEConv(4, 4, fanout=bad)
    for bad in (2.5, "5", True):
        with pytest.raises(TypeError, match="fanout"):
            sage.SAGEConv(4, 4, fanout=bad)
    layer = sage.SAGEConv(4, 6, aggr="max", fanout=5, bias=False)
    assert layer.lin_self.bias is None and layer.lin_nbr.bias is None and layer.lin_nbr.weight.shape == (6, 4)
