"""C-ABI of node masks on the quantised tiled products (include/qgtc_bitnodes.h: qgtc_tiledmm2bit_nodes / qgtc_tiledmm2int_nodes and
their _t): the header parses with cabi.signatures(text) to the four entries and equals its own golden file, every entry is exported and
bound by cabi.load(), the six earlier headers, their golden files and ABI version 11 are untouched, and bad arguments are refused before
any device work in the stated order - those of the _scaled twin (a NULL row_scale is not one: it is the plain sum), then a short mask,
then a misaligned mask. Every call here carries a bad argument and a NULL stream: nothing is launched (no GPU needed)."""
import ctypes
import os

import pytest

from qgtc_ppopp22_amd import cabi
from test_cabi import _lines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("qgtc_tiledmm2bit_nodes", "qgtc_tiledmm2int_nodes", "qgtc_tiledmm2bit_t_nodes", "qgtc_tiledmm2int_t_nodes")
EINVAL, ESIZE, EALIGN = 1, 2, 3
V, I, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
WORDS = 4   # S128(100) * 4
BIG = 1 << 16


def bitnodes_signatures():
    with open(cabi.BITNODES_HEADER) as f:
        return cabi.signatures(f.read())


@pytest.fixture(scope="module")
def lib():
    return cabi.load()


@pytest.fixture(scope="module")
def p():
    b = (ctypes.c_uint32 * (BIG + 64))()
    addr = (ctypes.addressof(b) + 255) & ~255   # 256-byte aligned address inside the buffer
    yield addr
    del b


def test_the_header_parses_to_the_four_entries():
    sig = bitnodes_signatures()
    assert list(sig) == list(ENTRIES)
    scaled = cabi.signatures()
    for name in ENTRIES:
        # each entry is its _scaled twin plus the (row_mask, nbr_mask, mask_words) of the _nodes entries, before the stream
        ret, args = scaled[name[:-len("_nodes")] + "_scaled"]
        assert sig[name] == (ret, args[:-1] + [V, V, Z, V]), name
    assert scaled["qgtc_tiledmm_f32_nodes"][1][-4:] == [V, V, Z, V]


def test_the_golden_file_holds():
    golden = open(os.path.join(ROOT, "tests", "golden", "qgtc_bitnodes_abi.txt")).read().splitlines()
    assert _lines(bitnodes_signatures()) == golden and len(golden) == 4


def test_every_entry_is_exported_and_bound(lib):
    for name, (ret, args) in bitnodes_signatures().items():
        fn = getattr(lib, name)
        assert fn.restype is ret and list(fn.argtypes) == args, name


def test_the_earlier_headers_are_untouched(lib):
    headers = ((cabi.HEADER, "qgtc_abi.txt"), (cabi.HEADS_HEADER, "qgtc_heads_abi.txt"), (cabi.ATTN_HEADS_HEADER, "qgtc_attn_heads_abi.txt"),
               (cabi.ADDSCORE_HEADER, "qgtc_addscore_abi.txt"), (cabi.FANOUT_HEADER, "qgtc_fanout_abi.txt"),
               (cabi.BLOCKS_HEADER, "qgtc_blocks_abi.txt"))
    golden = os.path.join(ROOT, "tests", "golden")
    for header, name in headers:
        text = open(header).read()
        assert not set(cabi.signatures(text)) & set(ENTRIES), header
        assert _lines(cabi.signatures(text)) == open(os.path.join(golden, name)).read().splitlines(), name
    assert lib.qgtc_abi_version() == 11
    assert "#define QGTC_ABI_VERSION 11" in open(cabi.HEADER).read()


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("which", ["bit", "int"])
def test_the_entries_refuse_bad_arguments_in_the_stated_order(lib, p, which, transposed):
    entry = getattr(lib, f"qgtc_tiledmm2{which}{'_t' if transposed else ''}_nodes")
    w = 4 if transposed else 3   # the index pointers and the tile words
    full = 4 * 104 * 4 if which == "bit" else 100 * 8    # 4 planes x PAD8(100) rows x 4 words, or 100 x 8 floats

    def f(idx=(p,) * w, T=1, n=100, N=8, b=2, ob=4, X=p, scale=p, out=p, size=BIG, rm=p, nm=p, mw=WORDS):
        args = list(idx) + [T, n, X, BIG, N, b] + ([ob] if which == "bit" else []) + [scale, out, size, rm, nm, mw, None]
        return entry(*args)

    # the twin's refusals, under masks, under one mask and under none, with and without a row_scale
    for kw in (dict(), dict(nm=None), dict(rm=None, nm=None, mw=0), dict(scale=None), dict(scale=None, rm=None)):
        assert f(n=0, **kw) == EINVAL and f(n=(1 << 23) + 1, **kw) == EINVAL and f(N=0, **kw) == EINVAL
        assert f(b=0, **kw) == EINVAL and f(b=9, **kw) == EINVAL and f(T=-1, **kw) == EINVAL
        assert f(X=None, **kw) == EINVAL and f(out=None, **kw) == EINVAL
        for i in range(w):
            assert f(idx=tuple(None if j == i else p for j in range(w)), **kw) == EINVAL, i
        # the bit kernels read row_ptr / col_ptr without looking at n_tiles: wanted even for an adjacency without tiles
        assert f(idx=(None,) * w, T=0, **kw) == EINVAL
        assert f(X=p + 4, **kw) == EALIGN and f(out=p + 4, **kw) == EALIGN and f(idx=(p,) * (w - 1) + (p + 4,), **kw) == EALIGN
        assert f(size=full - 1, **kw) == ESIZE and f(size=0, **kw) == ESIZE
        if which == "bit":
            assert f(ob=0, **kw) == EINVAL and f(ob=33, **kw) == EINVAL
            assert f(X=p + 4, ob=33, **kw) == EALIGN          # the shared check (invalid, then misaligned) before output_bit
        assert f(b=9, size=0, **kw) == EINVAL and f(X=p + 4, size=0, **kw) == EALIGN
    # then the masks': short when one is given, then misaligned
    for kw in (dict(rm=p, nm=None), dict(rm=None, nm=p), dict(rm=p, nm=p)):
        assert f(**kw, mw=WORDS - 1) == ESIZE and f(**kw, mw=0) == ESIZE, kw
        assert f(**kw, mw=WORDS - 1, scale=None) == ESIZE, kw
    assert f(rm=p + 4) == EALIGN and f(nm=p + 8) == EALIGN and f(rm=p + 1) == EALIGN and f(rm=None, nm=p + 4, scale=None) == EALIGN
    assert f(rm=p + 4, mw=WORDS - 1) == ESIZE                 # the length before the alignment
    # the twin's come first
    assert f(rm=p + 4, n=0) == EINVAL and f(mw=0, X=None) == EINVAL
    assert f(rm=p + 4, X=p + 4) == EALIGN and f(mw=0, out=p + 4) == EALIGN
    assert f(rm=p + 4, size=full - 1) == ESIZE and f(mw=0, size=full - 1) == ESIZE
    # an adjacency without tiles (its index pointer alone) is still checked
    none = dict(idx=(p,) + (None,) * (w - 1), T=0)
    assert f(**none, N=0) == EINVAL and f(**none, X=p + 4) == EALIGN and f(**none, size=0) == ESIZE
    assert f(**none, mw=1) == ESIZE and f(**none, nm=p + 4) == EALIGN
