"""C-ABI of the byte-code route (include/qgtc_codes.h: qgtc_affine_codes, qgtc_tiledmm_u8, qgtc_tiledmm_u8_t, qgtc_tiledmm_u8_affine,
qgtc_tiledmm_u8_t_affine): the header parses with cabi.signatures(text) to the five entries and equals its own golden file, every entry is
exported and bound by cabi.load(), the eight earlier headers, their golden files and ABI version 11 are untouched, and bad arguments are
refused before any device work in the stated order: invalid, then misaligned (a code matrix's stride below its width or off a multiple of
4 and a base off a 4-byte boundary included), then short. Every call here carries a bad argument and a NULL stream: nothing is launched
(no GPU needed)."""
import ctypes
import os

import pytest

from qgtc_ppopp22_amd import cabi
from test_cabi import _lines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("qgtc_affine_codes", "qgtc_tiledmm_u8", "qgtc_tiledmm_u8_t", "qgtc_tiledmm_u8_affine", "qgtc_tiledmm_u8_t_affine")
EINVAL, ESIZE, EALIGN = 1, 2, 3
V, I, Z, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_int64
BIG = 1 << 16


def codes_signatures():
    with open(cabi.CODES_HEADER) as f:
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


def test_the_header_parses_to_the_five_entries():
    sig = codes_signatures()
    assert list(sig) == list(ENTRIES)
    assert sig["qgtc_affine_codes"] == (I, [V, I, I, I, V, I, V, Z, Z, V])
    assert sig["qgtc_tiledmm_u8"] == (I, [V, V, V, L, I, V, Z, Z, I, V, Z, V, V, Z, V])
    assert sig["qgtc_tiledmm_u8_t"] == (I, [V, V, V, V, L, I, V, Z, Z, I, V, Z, V, V, Z, V])
    assert sig["qgtc_tiledmm_u8_affine"] == (I, [V, V, V, L, I, V, Z, Z, I, V, V, V, Z, V, V, Z, V])
    assert sig["qgtc_tiledmm_u8_t_affine"] == (I, [V, V, V, V, L, I, V, Z, Z, I, V, V, V, Z, V, V, Z, V])
    assert all(args[-1] is V for _, args in sig.values())    # the stream comes last


def test_the_golden_file_holds():
    golden = open(os.path.join(ROOT, "tests", "golden", "qgtc_codes_abi.txt")).read().splitlines()
    assert _lines(codes_signatures()) == golden and len(golden) == 5


def test_every_entry_is_exported_and_bound(lib):
    for name, (ret, args) in codes_signatures().items():
        fn = getattr(lib, name)
        assert fn.restype is ret and list(fn.argtypes) == args, name


def test_the_earlier_headers_are_untouched(lib):
    headers = ((cabi.HEADER, "qgtc_abi.txt"), (cabi.HEADS_HEADER, "qgtc_heads_abi.txt"), (cabi.ATTN_HEADS_HEADER, "qgtc_attn_heads_abi.txt"),
               (cabi.ADDSCORE_HEADER, "qgtc_addscore_abi.txt"), (cabi.FANOUT_HEADER, "qgtc_fanout_abi.txt"),
               (cabi.BLOCKS_HEADER, "qgtc_blocks_abi.txt"), (cabi.BITNODES_HEADER, "qgtc_bitnodes_abi.txt"),
               (cabi.AFFINE_HEADER, "qgtc_affine_abi.txt"))
    golden = os.path.join(ROOT, "tests", "golden")
    for header, name in headers:
        text = open(header).read()
        assert not set(cabi.signatures(text)) & set(ENTRIES), header
        assert _lines(cabi.signatures(text)) == open(os.path.join(golden, name)).read().splitlines(), name
    assert lib.qgtc_abi_version() == 11
    assert "#define QGTC_ABI_VERSION 11" in open(cabi.HEADER).read()


def test_codes_refuses_bad_arguments_in_the_stated_order(lib, p):
    H, W = 100, 62                       # PAD4(W) = 64
    need = (H - 1) * 64 + 64

    def f(x=p, H=H, W=W, b=4, qp=p, g=1, out=p, ld=64, on=need):
        return lib.qgtc_affine_codes(x, H, W, b, qp, g, out, ld, on, None)

    for kw in (dict(), dict(g=W)):
        assert f(x=None, **kw) == EINVAL and f(qp=None, **kw) == EINVAL and f(out=None, **kw) == EINVAL
        assert f(H=0, **kw) == EINVAL and f(W=0, **kw) == EINVAL and f(W=-1, **kw) == EINVAL
        assert f(b=0, **kw) == EINVAL and f(b=9, **kw) == EINVAL
        assert f(qp=p + 4, **kw) == EALIGN and f(qp=p + 8, **kw) == EALIGN
        assert f(out=p + 1, **kw) == EALIGN and f(out=p + 2, **kw) == EALIGN and f(out=p + 3, **kw) == EALIGN
        assert f(ld=60, **kw) == EALIGN and f(ld=61, **kw) == EALIGN and f(ld=63, **kw) == EALIGN and f(ld=66, **kw) == EALIGN
        assert f(ld=0, **kw) == EALIGN
        assert f(on=need - 1, **kw) == ESIZE and f(on=0, **kw) == ESIZE
        assert f(ld=128, **kw) == ESIZE and f(ld=128, on=(H - 1) * 128 + 63, **kw) == ESIZE
    for g in (0, 2, W - 1, W + 1, H, -1):
        assert f(g=g) == EINVAL, g
    # invalid before misaligned before short; a 4-byte aligned out is enough
    assert f(g=2, out=p + 1) == EINVAL and f(b=9, ld=61) == EINVAL and f(H=0, on=0) == EINVAL
    assert f(out=p + 2, on=0) == EALIGN and f(ld=60, on=0) == EALIGN and f(qp=p + 4, on=0) == EALIGN
    assert f(out=p + 4, on=0) == ESIZE


def _view(transposed, p):
    return (p, p, p, p) if transposed else (p, p, p)      # the view's index pointers, then tiles


@pytest.mark.parametrize("affine", [False, True], ids=["int", "affine"])
@pytest.mark.parametrize("transposed", [False, True], ids=["adj", "adjT"])
def test_the_products_refuse_bad_arguments_in_the_stated_order(lib, p, transposed, affine):
    n, N = 300, 62                       # PAD4(N) = 64, S128(n) * 4 = 12 mask words
    need = (n - 1) * 64 + 64
    fn = getattr(lib, "qgtc_tiledmm_u8" + ("_t" if transposed else "") + ("_affine" if affine else ""))
    nptr = 4 if transposed else 3

    def f(view=None, T=5, n=n, Q=p, ld=64, qn=need, N=N, qp=p, rs=p, out=p, on=n * N, rm=p, sm=p, mw=12):
        view = _view(transposed, p) if view is None else view
        mid = (qp, rs) if affine else ()
        return fn(*view, T, n, Q, ld, qn, N, *mid, out, on, rm, sm, mw, None)

    for kw in (dict(), dict(rm=None), dict(sm=None), dict(rm=None, sm=None, mw=0), dict(rs=None)):
        assert f(Q=None, **kw) == EINVAL and f(out=None, **kw) == EINVAL
        assert f(N=0, **kw) == EINVAL and f(N=-1, **kw) == EINVAL
        assert f(n=0, **kw) == EINVAL and f(n=(1 << 23) + 1, **kw) == EINVAL and f(T=-1, **kw) == EINVAL
        for k in range(nptr):            # tiles given, an index pointer or the tiles missing
            view = list(_view(transposed, p))
            view[k] = None
            assert f(view=tuple(view), **kw) == EINVAL, k
        if affine:
            assert f(qp=None, **kw) == EINVAL
            assert f(qp=p + 4, **kw) == EALIGN and f(qp=p + 8, **kw) == EALIGN
            if kw.get("rs", p) is not None:
                assert f(**{**kw, "rs": p + 2}) == EALIGN
        assert f(Q=p + 1, **kw) == EALIGN and f(Q=p + 2, **kw) == EALIGN and f(Q=p + 3, **kw) == EALIGN
        assert f(ld=60, **kw) == EALIGN and f(ld=61, **kw) == EALIGN and f(ld=63, **kw) == EALIGN and f(ld=66, **kw) == EALIGN
        assert f(out=p + 2, **kw) == EALIGN
        view = list(_view(transposed, p))
        view[-1] = p + 4                 # tiles off a 16-byte boundary
        assert f(view=tuple(view), **kw) == EALIGN
        assert f(qn=need - 1, **kw) == ESIZE and f(qn=0, **kw) == ESIZE and f(on=n * N - 1, **kw) == ESIZE and f(on=0, **kw) == ESIZE
        assert f(ld=128, **kw) == ESIZE
    assert f(rm=p + 4) == EALIGN and f(sm=p + 8) == EALIGN and f(rm=p + 4, sm=None) == EALIGN
    assert f(mw=11) == ESIZE and f(mw=0) == ESIZE and f(mw=11, rm=None) == ESIZE and f(mw=11, sm=None) == ESIZE
    # an adjacency without tiles may come with NULL index pointers: these reach the size check
    assert f(view=(None,) * nptr, T=0, on=0) == ESIZE
    # invalid before misaligned before short
    assert f(N=0, Q=p + 1) == EINVAL and f(Q=None, ld=61) == EINVAL and f(n=0, on=0) == EINVAL
    assert f(Q=p + 1, on=0) == EALIGN and f(ld=60, qn=0) == EALIGN and f(rm=p + 4, mw=0) == EALIGN and f(out=p + 2, mw=0) == EALIGN
    assert f(Q=p + 4, qn=0) == ESIZE
