"""C-ABI of affine quantisation (include/qgtc_affine.h: qgtc_affine_work_words, qgtc_affine_qparams, qgtc_val2bit_affine,
qgtc_affine_dequant): the header parses with cabi.signatures(text) to the four entries and equals its own golden file, every entry is
exported and bound by cabi.load(), the seven earlier headers, their golden files and ABI version 11 are untouched, and bad arguments are
refused before any device work in the stated order: invalid, then misaligned, then short. Every call here carries a bad argument and a
NULL stream: nothing is launched (no GPU needed)."""
import ctypes
import os

import pytest

from qgtc_ppopp22_amd import cabi
from test_cabi import _lines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("qgtc_affine_work_words", "qgtc_affine_qparams", "qgtc_val2bit_affine", "qgtc_affine_dequant")
EINVAL, ESIZE, EALIGN = 1, 2, 3
V, I, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
BIG = 1 << 16


def affine_signatures():
    with open(cabi.AFFINE_HEADER) as f:
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
    sig = affine_signatures()
    assert list(sig) == list(ENTRIES)
    assert sig["qgtc_affine_work_words"] == (Z, [I, I, I])
    assert sig["qgtc_affine_qparams"] == (I, [V, I, I, I, I, V, Z, V, Z, V])
    assert sig["qgtc_val2bit_affine"] == (I, [V, I, I, I, I, V, I, V, Z, V, Z, V])
    assert sig["qgtc_affine_dequant"] == (I, [V, I, I, I, V, V, V, I, V, V, V, I, V, Z, V])
    assert all(args[-1] is V for name, (_, args) in sig.items() if name != "qgtc_affine_work_words")    # the stream comes last


def test_the_golden_file_holds():
    golden = open(os.path.join(ROOT, "tests", "golden", "qgtc_affine_abi.txt")).read().splitlines()
    assert _lines(affine_signatures()) == golden and len(golden) == 4


def test_every_entry_is_exported_and_bound(lib):
    for name, (ret, args) in affine_signatures().items():
        fn = getattr(lib, name)
        assert fn.restype is ret and list(fn.argtypes) == args, name


def test_the_earlier_headers_are_untouched(lib):
    headers = ((cabi.HEADER, "qgtc_abi.txt"), (cabi.HEADS_HEADER, "qgtc_heads_abi.txt"), (cabi.ATTN_HEADS_HEADER, "qgtc_attn_heads_abi.txt"),
               (cabi.ADDSCORE_HEADER, "qgtc_addscore_abi.txt"), (cabi.FANOUT_HEADER, "qgtc_fanout_abi.txt"),
               (cabi.BLOCKS_HEADER, "qgtc_blocks_abi.txt"), (cabi.BITNODES_HEADER, "qgtc_bitnodes_abi.txt"))
    golden = os.path.join(ROOT, "tests", "golden")
    for header, name in headers:
        text = open(header).read()
        assert not set(cabi.signatures(text)) & set(ENTRIES), header
        assert _lines(cabi.signatures(text)) == open(os.path.join(golden, name)).read().splitlines(), name
    assert lib.qgtc_abi_version() == 11
    assert "#define QGTC_ABI_VERSION 11" in open(cabi.HEADER).read()


def test_the_work_words(lib):
    w = lib.qgtc_affine_work_words
    assert w(0, 5, 0) == 0 and w(5, 0, 1) == 0 and w(-1, 5, 0) == 0
    assert w(1, 1, 0) == 2 and w(64, 64, 0) == 2 and w(64, 65, 0) == 4        # one pair per 4096 elements
    assert w(1 << 15, 1 << 15, 0) == 2048                                     # 1024 workgroups at the most
    assert w(1, 7, 1) == 14 and w(33, 5, 1) == 2 * 2 * 5 and w(1 << 20, 3, 1) == 2 * 64 * 3    # one pair per 32-row slice and column, 64 slices at the most


def test_qparams_refuses_bad_arguments_in_the_stated_order(lib, p):
    need = lib.qgtc_affine_work_words(100, 64, 1)

    def f(x=p, H=100, W=64, b=4, pc=1, qp=p, qn=4 * 64, work=p, wn=need):
        return lib.qgtc_affine_qparams(x, H, W, b, pc, qp, qn, work, wn, None)

    for kw in (dict(), dict(pc=0, qn=4, wn=lib.qgtc_affine_work_words(100, 64, 0))):
        assert f(x=None, **kw) == EINVAL and f(qp=None, **kw) == EINVAL and f(work=None, **kw) == EINVAL
        assert f(H=0, **kw) == EINVAL and f(W=0, **kw) == EINVAL and f(H=-3, **kw) == EINVAL
        assert f(b=0, **kw) == EINVAL and f(b=9, **kw) == EINVAL
        assert f(**{**kw, "qp": p + 4}) == EALIGN and f(**{**kw, "qp": p + 8}) == EALIGN
        assert f(**{**kw, "qn": kw.get("qn", 4 * 64) - 1}) == ESIZE and f(**{**kw, "wn": kw.get("wn", need) - 1}) == ESIZE
        assert f(**{**kw, "wn": 0}) == ESIZE
    # invalid before misaligned before short
    assert f(b=9, qp=p + 4) == EINVAL and f(H=0, qn=0) == EINVAL
    assert f(qp=p + 4, qn=0) == EALIGN and f(qp=p + 4, wn=0) == EALIGN


@pytest.mark.parametrize("col_major", [0, 1])
def test_val2bit_affine_refuses_bad_arguments_in_the_stated_order(lib, p, col_major):
    H, W, b = 100, 64, 4
    full = lib.qgtc_cols_words(H, W, b, 0) if col_major else lib.qgtc_rows_words(H, W, b)
    lines = W if col_major else H

    def f(x=p, H=H, W=W, b=b, qp=p, g=1, out=p, on=BIG, sums=p, sn=BIG):
        return lib.qgtc_val2bit_affine(x, H, W, b, col_major, qp, g, out, on, sums, sn, None)

    for kw in (dict(), dict(g=W), dict(sums=None, sn=0)):
        assert f(x=None, **kw) == EINVAL and f(qp=None, **kw) == EINVAL and f(out=None, **kw) == EINVAL
        assert f(H=0, **kw) == EINVAL and f(W=0, **kw) == EINVAL and f(W=-1, **kw) == EINVAL
        assert f(b=0, **kw) == EINVAL and f(b=9, **kw) == EINVAL
        assert f(out=p + 4, **kw) == EALIGN and f(qp=p + 4, **kw) == EALIGN and f(out=p + 8, **kw) == EALIGN
        assert f(on=full - 1, **kw) == ESIZE and f(on=0, **kw) == ESIZE
    for g in (0, 2, W - 1, W + 1, H, -1):
        assert f(g=g) == EINVAL, g
    assert f(sn=lines - 1) == ESIZE and f(sn=0) == ESIZE
    # invalid before misaligned before short; x needs no 16-byte alignment
    assert f(g=2, out=p + 4) == EINVAL and f(b=9, on=0) == EINVAL
    assert f(out=p + 4, on=0) == EALIGN and f(qp=p + 4, sn=0) == EALIGN
    assert f(x=p + 4, on=0) == ESIZE


def test_dequant_refuses_bad_arguments_in_the_stated_order(lib, p):
    M, N = 33, 7

    def f(acc=p, M=M, N=N, K=20, qa=p, rs=p, qb=p, g=N, cs=p, scale=p, bias=p, relu=1, out=p, on=M * N):
        return lib.qgtc_affine_dequant(acc, M, N, K, qa, rs, qb, g, cs, scale, bias, relu, out, on, None)

    for kw in (dict(), dict(g=1), dict(rs=None, cs=None, scale=None, bias=None, relu=0)):
        assert f(acc=None, **kw) == EINVAL and f(qa=None, **kw) == EINVAL and f(qb=None, **kw) == EINVAL and f(out=None, **kw) == EINVAL
        assert f(M=0, **kw) == EINVAL and f(N=0, **kw) == EINVAL and f(K=0, **kw) == EINVAL and f(K=-1, **kw) == EINVAL
        assert f(qa=p + 4, **kw) == EALIGN and f(qb=p + 8, **kw) == EALIGN
        assert f(on=M * N - 1, **kw) == ESIZE and f(on=0, **kw) == ESIZE
    for g in (0, 2, N - 1, N + 1, M):
        assert f(g=g) == EINVAL, g
    assert f(g=2, qa=p + 4) == EINVAL and f(K=0, on=0) == EINVAL
    assert f(qa=p + 4, on=0) == EALIGN
