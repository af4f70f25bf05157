"""C-ABI of mini-batch sampling (include/qgtc_blocks.h: the two masked selection entries, the two frontier entries and the _fanout_nodes
twins of the eight _fanout entries): the header parses with cabi.signatures(text) to the 12 entries, every entry is exported and bound by
cabi.load(), the header's own golden file holds, the five earlier headers, their golden files and ABI version 11 are untouched, bad
arguments are refused before any device work in the project's order - invalid, then misaligned, then short, the node masks' refusals after
the twin's -, and the Python layer refuses a bad masked sample and still refuses the keywords it refused (no GPU needed)."""
import ctypes
import os

import pytest

from qgtc_ppopp22_amd import cabi
from test_cabi import _lines
from test_tiled_fanout_abi import EALIGN, EINVAL, ESIZE, TWINS, _adjacency, _twin_call, fanout_signatures

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELECT = ("qgtc_tiled_fanout_thr_nodes", "qgtc_tiled_fanout_thr_t_nodes")
FRONTIER = ("qgtc_tiled_fanout_frontier", "qgtc_tiled_fanout_frontier_t")
ENTRIES = SELECT + FRONTIER + tuple(t + "_fanout_nodes" for t in TWINS)
V, I, Z, P64, U64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_int64, ctypes.c_uint64
WORDS = 4   # S128(100) * 4


def blocks_signatures():
    with open(cabi.BLOCKS_HEADER) as f:
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


def test_the_header_parses_to_the_twelve_entries():
    sig = blocks_signatures()
    assert list(sig) == list(ENTRIES) and len(sig) == 12
    fan = fanout_signatures()
    # the selection: the parent's arguments, then (kept, kept_elems, row_mask, nbr_mask, mask_words)
    for name in SELECT:
        ret, args = fan[name[:-len("_nodes")]]
        assert sig[name] == (ret, args[:-1] + [V, Z, V, V, Z, V]), name
    assert sig[FRONTIER[0]] == (I, [V, V, V, V, P64, I, V, U64, V, V, V, Z, V, Z, V])
    assert sig[FRONTIER[1]] == (I, [V, V, V, P64, I, V, U64, V, V, V, Z, V, Z, V])
    # each twin is its _fanout twin plus the (row_mask, nbr_mask, mask_words) of the _nodes entries
    nodes = cabi.signatures()
    for t in TWINS:
        ret, args = fan[t + "_fanout"]
        assert nodes[t + "_nodes"][1][-4:] == [V, V, Z, V]
        assert sig[t + "_fanout_nodes"] == (ret, args[:-1] + [V, V, Z, V]), t


def test_the_golden_file_holds():
    golden = open(os.path.join(ROOT, "tests", "golden", "qgtc_blocks_abi.txt")).read().splitlines()
    assert _lines(blocks_signatures()) == golden and len(golden) == 12


def test_every_entry_is_exported_and_bound(lib):
    for name, (ret, args) in blocks_signatures().items():
        fn = getattr(lib, name)
        assert fn.restype is ret and list(fn.argtypes) == args, name


def test_the_earlier_headers_are_untouched(lib):
    texts = {h: open(h).read() for h in (cabi.HEADER, cabi.HEADS_HEADER, cabi.ATTN_HEADS_HEADER, cabi.ADDSCORE_HEADER, cabi.FANOUT_HEADER)}
    for text in texts.values():
        assert not set(cabi.signatures(text)) & set(ENTRIES) and "frontier" not in text and "fanout_nodes" not in text
    assert lib.qgtc_abi_version() == 11
    assert "#define QGTC_ABI_VERSION 11" in texts[cabi.HEADER]
    golden = os.path.join(ROOT, "tests", "golden")
    for header, name in ((cabi.HEADER, "qgtc_abi.txt"), (cabi.HEADS_HEADER, "qgtc_heads_abi.txt"),
                         (cabi.ATTN_HEADS_HEADER, "qgtc_attn_heads_abi.txt"), (cabi.ADDSCORE_HEADER, "qgtc_addscore_abi.txt"),
                         (cabi.FANOUT_HEADER, "qgtc_fanout_abi.txt")):
        assert _lines(cabi.signatures(texts[header])) == open(os.path.join(golden, name)).read().splitlines(), name


def _mask_refusals(f, p, short):
    """the node masks' refusals of f(rm=, nm=, mw=), made after the twin's: `short` is a twin-side size refusal. Every call here carries
    a bad argument: a call without one would launch."""
    for kw in (dict(rm=p, nm=None), dict(rm=None, nm=p), dict(rm=p, nm=p)):
        assert f(**kw, mw=WORDS - 1) == ESIZE and f(**kw, mw=0) == ESIZE, kw
    assert f(rm=p + 4) == EALIGN and f(nm=p + 8) == EALIGN and f(rm=p + 1) == EALIGN
    assert f(rm=p + 4, mw=WORDS - 1) == ESIZE                       # tiled_nodes_args_ok looks at the length first
    # the twin's refusals come first
    assert f(rm=p + 4, n=0) == EINVAL and f(mw=0, thr=None) == EINVAL
    assert f(rm=p + 4, thr=p + 2) == EALIGN and f(mw=0, thr=p + 2) == EALIGN
    assert f(rm=p + 4, **short) == ESIZE


@pytest.mark.parametrize("transposed", [False, True])
def test_the_masked_selection_refuses_bad_arguments(lib, p, transposed):
    entry = getattr(lib, SELECT[transposed])
    w = 4 if transposed else 3

    def f(idx=(p,) * w, T=2, n=100, k=3, seed=1, thr=p, te=100, kept=p, ke=100, rm=p, nm=p, mw=WORDS):
        return entry(*idx, T, n, k, seed, thr, te, kept, ke, rm, nm, mw, None)

    assert f(n=0) == EINVAL and f(n=(1 << 23) + 1) == EINVAL and f(T=-1) == EINVAL
    assert f(k=0) == EINVAL and f(k=-1) == EINVAL and f(thr=None) == EINVAL
    for i in range(w):
        assert f(idx=tuple(None if j == i else p for j in range(w))) == EINVAL
    assert f(idx=(p,) * (w - 1) + (p + 4,)) == EALIGN and f(thr=p + 2) == EALIGN
    assert f(kept=p + 2) == EALIGN and f(kept=p + 1, ke=0) == EALIGN
    assert f(te=99) == ESIZE and f(te=0) == ESIZE and f(ke=99) == ESIZE
    # the order: invalid before misaligned before short
    assert f(kept=p + 2, k=0) == EINVAL and f(kept=p + 2, thr=None) == EINVAL
    assert f(te=99, kept=p + 2) == EALIGN and f(ke=99, thr=p + 2) == EALIGN and f(ke=99, k=0) == EINVAL
    _mask_refusals(f, p, dict(ke=99))
    # an adjacency without tiles is still checked
    none = dict(idx=(None,) * w, T=0)
    assert f(**none, k=0) == EINVAL and f(**none, kept=p + 2) == EALIGN and f(**none, ke=99) == ESIZE and f(**none, mw=1) == ESIZE


@pytest.mark.parametrize("transposed", [False, True])
def test_the_frontier_refuses_bad_arguments(lib, p, transposed):
    entry = getattr(lib, FRONTIER[transposed])
    w = 3 if transposed else 4   # the OTHER view's index: the column index for a row-axis sample

    def f(idx=(p,) * w, T=2, n=100, thr=p, seed=1, rm=p, nm=p, inc=p, mw=WORDS, out=p, ow=WORDS):
        return entry(*idx, T, n, thr, seed, rm, nm, inc, mw, out, ow, None)

    assert f(n=0) == EINVAL and f(n=(1 << 23) + 1) == EINVAL and f(T=-1) == EINVAL and f(thr=None) == EINVAL and f(out=None) == EINVAL
    for i in range(w):
        assert f(idx=tuple(None if j == i else p for j in range(w))) == EINVAL
    assert f(idx=(p,) * (w - 1) + (p + 4,)) == EALIGN and f(thr=p + 2) == EALIGN
    for name in ("rm", "nm", "inc", "out"):
        for off in (1, 4, 8):
            assert f(**{name: p + off}) == EALIGN, (name, off)
    assert f(ow=WORDS - 1) == ESIZE and f(ow=0) == ESIZE and f(mw=WORDS - 1) == ESIZE
    for kw in (dict(rm=p, nm=None, inc=None), dict(rm=None, nm=p, inc=None), dict(rm=None, nm=None, inc=p)):
        assert f(**kw, mw=0) == ESIZE, kw
    # the order
    assert f(out=p + 4, thr=None) == EINVAL and f(ow=0, n=0) == EINVAL and f(ow=0, out=p + 4) == EALIGN and f(mw=0, inc=p + 4) == EALIGN
    # an adjacency without tiles is still checked
    none = dict(idx=(None,) * w, T=0)
    assert f(**none, out=None) == EINVAL and f(**none, out=p + 4) == EALIGN and f(**none, ow=3) == ESIZE


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("stem", ["qgtc_tiledmm_f32", "qgtc_tiledmax_f32", "qgtc_tiledatt_f32", "qgtc_tiledatt_grad_f32"])
def test_the_twins_refuse_what_their_fanout_twins_refuse_and_bad_masks(lib, p, stem, transposed):
    """The _fanout twin's refusals are checked by its own test's code, run on the _fanout_nodes entry with the masks appended."""
    import test_tiled_fanout_abi as parent

    class Masked:
        """the library with every _fanout entry answered by its _fanout_nodes twin under the masks given"""

        def __init__(self, *masks):
            self.masks = masks

        def __getattr__(self, name):
            fn = getattr(lib, name + "_nodes")
            return lambda *a: fn(*a[:-1], *self.masks, a[-1])   # before the stream

    parent.test_the_twins_refuse_bad_arguments(Masked(p, p, WORDS), p, stem, transposed)
    parent.test_the_twins_refuse_bad_arguments(Masked(None, None, 0), p, stem, transposed)
    sizes = _twin_call(lib, p, stem, transposed)[3]

    def f(rm=p, nm=p, mw=WORDS, **kw):
        return _twin_call(Masked(rm, nm, mw), p, stem, transposed)[0](**kw)

    _mask_refusals(f, p, {sizes[0]: 99})


# ---- the Python layer ----------------------------------------------------------------------------------------------------------------------
def test_a_hand_built_masked_sample_is_checked_before_any_launch():
    import torch

    from qgtc_ppopp22_amd import fanout as fo

    tiled, adj, X = _adjacency()
    n = adj.n
    thr, counts, mask = torch.zeros(n, dtype=torch.int32), torch.zeros(n, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    calls = (lambda **kw: tiled.tiledMMFloat(adj, X, **kw), lambda **kw: tiled.tiledAggregate(adj, X, reduce="max", **kw))
    bad_masks = ((mask.tolist(), TypeError, "torch.Tensor"), (mask.to(torch.int64), TypeError, "int32"), (mask[:-1], ValueError, "shape"),
                 (torch.zeros(8, dtype=torch.int32), ValueError, "shape"), (torch.zeros(8, dtype=torch.int32)[::2], ValueError, "contiguous"),
                 (mask.to("meta"), ValueError, "device"))
    bad_counts = ((counts.tolist(), TypeError, "torch.Tensor"), (counts.to(torch.int64), TypeError, "int32"),
                  (counts[:-1], ValueError, "shape"), (torch.zeros(2 * n, dtype=torch.int32)[::2], ValueError, "contiguous"),
                  (counts.to("meta"), ValueError, "device"))
    for call in calls:
        for name in ("row_mask", "nbr_mask"):
            for bad, error, match in bad_masks:
                with pytest.raises(error, match=f"FanoutSample's {name} must.*{match}"):
                    call(fanout=fo.FanoutSample(adj, 3, 1, thr, **{name: bad}))
        for bad, error, match in bad_counts:
            with pytest.raises(error, match=f"counts.*{match}"):
                call(fanout=fo.FanoutSample(adj, 3, 1, thr, mask, None, bad))
        with pytest.raises(ValueError, match="shape"):
            call(fanout=fo.FanoutSample(adj, 3, 1, thr[:-1], mask, mask, counts))
    # sample_fanout, frontier and sample_blocks check their own arguments
    for name in ("row_mask", "nbr_mask"):
        for bad, error, match in bad_masks:
            with pytest.raises(error, match=match):
                fo.sample_fanout(adj, 3, 1, **{name: bad})
    with pytest.raises(ValueError, match="k must be at least 1"):
        fo.sample_fanout(adj, 0, 1, row_mask=mask)
    with pytest.raises(TypeError, match="FanoutSample"):
        fo.frontier((3, 1))
    with pytest.raises(ValueError, match="include"):
        fo.frontier(fo.FanoutSample(adj, 3, 1, thr, mask, None, counts), include=mask[:-1])
    with pytest.raises(ValueError, match="shape"):
        fo.frontier(fo.FanoutSample(adj, 3, 1, thr, mask[:-1], None, counts))
    with pytest.raises(ValueError, match="seeds"):
        fo.sample_blocks(adj, mask[:-1], (3, 2), 1)
    with pytest.raises(ValueError, match="at least one layer"):
        fo.sample_blocks(adj, mask, (), 1)
    with pytest.raises(ValueError, match="k must be at least 1"):
        fo.sample_blocks(adj, mask, (3, 0), 1)
    with pytest.raises(TypeError, match="k must be an int"):
        fo.sample_blocks(adj, mask, (3, 2.0), 1)
    with pytest.raises(ValueError, match="seed"):
        fo.sample_blocks(adj, mask, (3, 2), -1)


def test_the_keyword_refusals_are_still_raised():
    """fanout= beside the KEYWORD row_mask= / nbr_mask= stays refused in the same words, with a pair and with a sample, masked or not:
    the masks of a mini-batch travel inside the sample."""
    import torch

    from qgtc_ppopp22_amd import fanout as fo

    tiled, adj, X = _adjacency()
    n = adj.n
    bitmap = torch.zeros(4, dtype=torch.int32)
    thr = torch.zeros(n, dtype=torch.int32)
    samples = ((3, 1), fo.FanoutSample(adj, 3, 1, thr), fo.FanoutSample(adj, 3, 1, thr, bitmap, bitmap, thr.clone()))
    for call in (lambda **kw: tiled.tiledMMFloat(adj, X, **kw), lambda **kw: tiled.tiledAggregate(adj, X, **kw)):
        for s in samples:
            for kw in (dict(row_mask=bitmap), dict(nbr_mask=bitmap), dict(row_mask=bitmap, nbr_mask=bitmap)):
                with pytest.raises(ValueError, match="fanout cannot be combined with row_mask / nbr_mask: not built"):
                    call(fanout=s, **kw)
            with pytest.raises(ValueError, match="fanout cannot be combined with edge_drop: not built"):
                call(fanout=s, edge_drop=(0.5, 1))
            with pytest.raises(ValueError, match="fanout cannot be combined with edge_weight: not built"):
                call(fanout=s, edge_weight=torch.zeros(0, dtype=torch.float32))
            with pytest.raises(ValueError, match=r"fanout cannot be combined with \[n, H\] scores: not built"):
                call(fanout=s, attn=(torch.zeros((n, 2)), torch.zeros((n, 2))))


def test_sageconv_refuses_a_bad_block():
    import torch

    from qgtc_ppopp22_amd import fanout as fo, sage

    tiled, adj, X = _adjacency()
    layer = sage.SAGEConv(4, 4)
    with pytest.raises(TypeError, match="fanout.Block"):
        layer(adj, X, block=(3, 1))
    _, other, _ = _adjacency()
    thr, mask = torch.zeros(adj.n, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="another view"):
        layer(adj, X, block=fo.Block(mask, fo.FanoutSample(other, 3, 1, thr, mask, None, thr.clone()), mask))
    with pytest.raises(ValueError, match="needs its counts"):
        fo.FanoutSample(adj, 3, 1, thr, mask).mean_scale()
