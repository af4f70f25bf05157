"""C-ABI of the multi-head entries (include/qgtc_heads.h: the per-edge dot, the weighted sum on both views, the edge softmax and its
gradient on both views, each with `int heads` before the stream): the header parses with cabi.signatures(text), every entry is exported
and bound by cabi.load(), the header's own golden file holds, qgtc.h's entries and ABI version are untouched, and bad arguments are
refused before any device work in the single-head entries' order - invalid, then misaligned, then short (no GPU needed)."""
import ctypes
import os

import pytest

from qgtc_ppopp22_amd import cabi
from test_cabi import _lines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, ESIZE, EALIGN = 0, 1, 2, 3
# the entry with heads -> the entry of qgtc.h it generalises
TWINS = {"qgtc_tiled_sddmm_heads_f32": "qgtc_tiled_sddmm_f32",
         "qgtc_tiledmm_f32_edge_heads": "qgtc_tiledmm_f32_edge",
         "qgtc_tiledmm_f32_t_edge_heads": "qgtc_tiledmm_f32_t_edge",
         "qgtc_tiled_edge_softmax_heads_f32": "qgtc_tiled_edge_softmax_f32",
         "qgtc_tiled_edge_softmax_heads_f32_t": "qgtc_tiled_edge_softmax_f32_t",
         "qgtc_tiled_edge_softmax_grad_heads_f32": "qgtc_tiled_edge_softmax_grad_f32",
         "qgtc_tiled_edge_softmax_grad_heads_f32_t": "qgtc_tiled_edge_softmax_grad_f32_t"}


def heads_signatures():
    with open(os.path.join(ROOT, "include", "qgtc_heads.h")) as f:
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


def test_the_header_parses_to_the_seven_entries_and_each_is_its_twin_plus_heads():
    sig, base = heads_signatures(), cabi.signatures()
    assert list(sig) == list(TWINS)
    for name, twin in TWINS.items():
        ret, args = sig[name]
        tret, targs = base[twin]
        assert ret is tret and args == targs[:-1] + [ctypes.c_int, ctypes.c_void_p], name   # ..., int heads, void *stream


def test_the_golden_file_holds():
    golden = open(os.path.join(ROOT, "tests", "golden", "qgtc_heads_abi.txt")).read().splitlines()
    assert _lines(heads_signatures()) == golden


def test_every_entry_is_exported_and_bound(lib):
    for name, (ret, args) in heads_signatures().items():
        fn = getattr(lib, name)
        assert fn.restype is ret and list(fn.argtypes) == args, name


def test_the_first_header_is_untouched(lib):
    sig = cabi.signatures()
    assert not set(sig) & set(TWINS), "cabi.signatures() stays include/qgtc.h's entries"
    assert "qgtc_heads" not in open(cabi.HEADER).read()
    assert lib.qgtc_abi_version() == 11
    assert "#define QGTC_ABI_VERSION 11" in open(cabi.HEADER).read()


def test_sddmm_refuses_bad_arguments(lib, p):
    big = 1 << 16

    def f(rp=p, kq=p, tl=p, T=2, n=100, A=p, B=p, ab=big, N=8, vp=p, vr=p, out=p, nv=9, heads=2):
        return lib.qgtc_tiled_sddmm_heads_f32(rp, kq, tl, T, n, A, B, ab, N, vp, vr, out, nv, heads, None)

    assert f(n=0) == EINVAL and f(n=(1 << 23) + 1) == EINVAL and f(N=0) == EINVAL and f(T=-1) == EINVAL
    for name in ("rp", "kq", "tl", "A", "B", "vp", "vr", "out"):
        assert f(**{name: None}) == EINVAL, name
    assert f(nv=1 << 31) == EINVAL
    assert f(heads=0) == EINVAL and f(heads=-1) == EINVAL and f(heads=3) == EINVAL and f(N=9) == EINVAL and f(heads=16) == EINVAL
    assert f(tl=p + 4) == EALIGN
    for name in ("A", "B", "out"):
        assert f(**{name: p + 2}) == EALIGN, name
    assert f(vp=p + 4) == EALIGN and f(vr=p + 1) == EALIGN
    assert f(ab=799) == ESIZE and f(ab=799, heads=8) == ESIZE and f(ab=799, heads=1) == ESIZE
    # the order: invalid before misaligned before short, heads among the invalid
    assert f(ab=799, A=p + 2) == EALIGN and f(ab=799, B=None) == EINVAL
    assert f(A=p + 2, heads=0) == EINVAL and f(ab=799, heads=3) == EINVAL and f(vr=p + 1, heads=5) == EINVAL
    assert f(n=1 << 23, ab=799) == ESIZE
    assert f(T=0, rp=None, kq=None, tl=None, vp=None, vr=None) == OK and f(nv=0, out=None) == OK   # nothing to do: no device work
    assert f(T=0, rp=None, kq=None, tl=None, vp=None, vr=None, heads=0) == EINVAL


@pytest.mark.parametrize("transposed", [False, True])
def test_weighted_products_refuse_bad_arguments(lib, p, transposed):
    entry = lib.qgtc_tiledmm_f32_t_edge_heads if transposed else lib.qgtc_tiledmm_f32_edge_heads
    k = 4 if transposed else 3
    big = 1 << 16

    def f(idx=(p,) * k, T=2, n=100, X=p, xe=big, N=8, rs=None, out=p, oe=big, vp=p, vr=p, vals=p, nv=9, heads=4):
        return entry(*idx, T, n, X, xe, N, rs, out, oe, vp, vr, vals, nv, heads, None)

    assert f(n=0) == EINVAL and f(n=(1 << 23) + 1) == EINVAL and f(N=0) == EINVAL and f(T=-1) == EINVAL
    assert f(X=None) == EINVAL and f(out=None) == EINVAL
    for i in range(k):
        assert f(idx=tuple(None if j == i else p for j in range(k))) == EINVAL
    for name in ("vp", "vr", "vals"):
        assert f(**{name: None}) == EINVAL, name
    assert f(nv=1 << 31) == EINVAL
    assert f(heads=0) == EINVAL and f(heads=-2) == EINVAL and f(heads=3) == EINVAL and f(N=10) == EINVAL
    assert f(idx=(p,) * (k - 1) + (p + 4,)) == EALIGN     # tiles off 16 bytes
    assert f(X=p + 2) == EALIGN and f(out=p + 2) == EALIGN and f(rs=p + 2) == EALIGN
    assert f(vp=p + 4) == EALIGN and f(vr=p + 1) == EALIGN and f(vals=p + 2) == EALIGN
    assert f(xe=799) == ESIZE and f(oe=799) == ESIZE and f(xe=799, heads=1) == ESIZE
    assert f(xe=799, vals=None) == EINVAL and f(xe=799, vp=p + 4) == EALIGN and f(X=p + 2, vr=None) == EINVAL
    assert f(xe=799, heads=0) == EINVAL and f(X=p + 2, heads=3) == EINVAL and f(N=0, heads=0) == EINVAL


@pytest.mark.parametrize("transposed", [False, True])
def test_softmax_refuses_bad_arguments(lib, p, transposed):
    entry = lib.qgtc_tiled_edge_softmax_heads_f32_t if transposed else lib.qgtc_tiled_edge_softmax_heads_f32
    k = 4 if transposed else 3

    def f(idx=(p,) * k, T=2, n=100, vp=p, vr=p, logits=p, alpha=p, nv=9, m=p, inv=p, heads=3):
        return entry(*idx, T, n, vp, vr, logits, alpha, nv, m, inv, heads, None)

    assert f(n=0) == EINVAL and f(n=(1 << 23) + 1) == EINVAL and f(T=-1) == EINVAL
    for i in range(k):
        assert f(idx=tuple(None if j == i else p for j in range(k))) == EINVAL, i
    for name in ("vp", "vr", "logits", "alpha"):
        assert f(**{name: None}) == EINVAL, name
    assert f(nv=1 << 31) == EINVAL
    assert f(heads=0) == EINVAL and f(heads=-1) == EINVAL and f(heads=65536) == EINVAL   # the heads ride a grid dimension
    assert f(heads=65535, vr=p + 1) == EALIGN                                              # in range: the next refusal is reached
    assert f(idx=(p,) * (k - 1) + (p + 4,)) == EALIGN
    assert f(vp=p + 4) == EALIGN and f(vr=p + 1) == EALIGN
    for name in ("logits", "alpha", "m", "inv"):
        assert f(**{name: p + 2}) == EALIGN, name
    assert f(logits=p + 2, vr=None) == EINVAL and f(n=0, m=p + 2) == EINVAL and f(alpha=p + 2, heads=0) == EINVAL
    # nothing to do, no device work: m and inv not wanted
    assert f(idx=(None,) * k, T=0, vp=None, vr=None, logits=None, alpha=None, nv=0, m=None, inv=None) == OK
    assert f(nv=0, logits=None, alpha=None, m=None, inv=None) == OK
    assert f(nv=0, logits=None, alpha=None, m=None, inv=None, heads=0) == EINVAL


@pytest.mark.parametrize("transposed", [False, True])
def test_softmax_gradient_refuses_bad_arguments(lib, p, transposed):
    entry = lib.qgtc_tiled_edge_softmax_grad_heads_f32_t if transposed else lib.qgtc_tiled_edge_softmax_grad_heads_f32
    k = 4 if transposed else 3

    def f(idx=(p,) * k, T=2, n=100, vp=p, vr=p, alpha=p, g=p, out=p, nv=9, heads=3):
        return entry(*idx, T, n, vp, vr, alpha, g, out, nv, heads, None)

    assert f(n=0) == EINVAL and f(n=(1 << 23) + 1) == EINVAL and f(T=-1) == EINVAL
    for i in range(k):
        assert f(idx=tuple(None if j == i else p for j in range(k))) == EINVAL, i
    for name in ("vp", "vr", "alpha", "g", "out"):
        assert f(**{name: None}) == EINVAL, name
    assert f(nv=1 << 31) == EINVAL and f(heads=0) == EINVAL and f(heads=65536) == EINVAL
    assert f(idx=(p,) * (k - 1) + (p + 4,)) == EALIGN
    assert f(vp=p + 4) == EALIGN and f(vr=p + 1) == EALIGN
    for name in ("alpha", "g", "out"):
        assert f(**{name: p + 2}) == EALIGN, name
    assert f(g=p + 2, vp=None) == EINVAL and f(vr=p + 1, out=None) == EINVAL and f(g=p + 2, heads=0) == EINVAL
    assert f(idx=(None,) * k, T=0, vp=None, vr=None, alpha=None, g=None, out=None, nv=0) == OK
    assert f(nv=0, alpha=None, g=None, out=None) == OK
