"""C-ABI of the additive edge score (include/qgtc_addscore.h: the score on the row view and its gradient folds on both views, each
with `int heads` before the stream): the header parses with cabi.signatures(text) to the three entries, every entry is exported and
bound by cabi.load(), the header's own golden file holds, the three earlier headers, their golden files and ABI version 11 are
untouched, and bad arguments are refused before any device work in the project's order - invalid, then misaligned, then short - for
heads in {1, 2}, with the refusals of `heads` themselves (no GPU needed)."""
import ctypes
import os

import pytest

from qgtc_ppopp22_amd import cabi
from test_cabi import _lines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, ESIZE, EALIGN = 0, 1, 2, 3
ENTRIES = ("qgtc_tiled_addscore_heads_f32", "qgtc_tiled_addscore_grad_heads_f32", "qgtc_tiled_addscore_grad_heads_f32_t")
V, I, Z, F, P64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_float, ctypes.c_int64


def addscore_signatures():
    with open(cabi.ADDSCORE_HEADER) as f:
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


def test_the_header_parses_to_the_three_entries():
    sig = addscore_signatures()
    assert list(sig) == list(ENTRIES)
    grad = [V, V, Z, I, V, Z, F, V, V, Z, V, V, V, Z, I, V]   # own, nbr, x_elems, N, att, att_elems, slope, d_own, P, out_elems, ...
    assert sig[ENTRIES[0]] == (I, [V, V, V, P64, I, V, V, Z, I, V, Z, F, V, V, V, Z, I, V])
    assert sig[ENTRIES[1]] == (I, [V, V, V, P64, I] + grad)
    assert sig[ENTRIES[2]] == (I, [V, V, V, V, P64, I] + grad)
    for name, (_, args) in sig.items():
        assert args[-2:] == [I, V], name   # ..., int heads, void *stream


def test_the_golden_file_holds():
    golden = open(os.path.join(ROOT, "tests", "golden", "qgtc_addscore_abi.txt")).read().splitlines()
    assert _lines(addscore_signatures()) == golden


def test_every_entry_is_exported_and_bound(lib):
    for name, (ret, args) in addscore_signatures().items():
        fn = getattr(lib, name)
        assert fn.restype is ret and list(fn.argtypes) == args, name


def test_the_earlier_headers_are_untouched(lib):
    sig = cabi.signatures()
    texts = {h: open(h).read() for h in (cabi.HEADER, cabi.HEADS_HEADER, cabi.ATTN_HEADS_HEADER)}
    for text in texts.values():
        assert not set(cabi.signatures(text)) & set(ENTRIES) and "addscore" not in text
    assert lib.qgtc_abi_version() == 11
    assert "#define QGTC_ABI_VERSION 11" in texts[cabi.HEADER]
    golden = os.path.join(ROOT, "tests", "golden")
    assert _lines(sig) == open(os.path.join(golden, "qgtc_abi.txt")).read().splitlines()
    assert _lines(cabi.signatures(texts[cabi.HEADS_HEADER])) == open(os.path.join(golden, "qgtc_heads_abi.txt")).read().splitlines()
    assert _lines(cabi.signatures(texts[cabi.ATTN_HEADS_HEADER])) == open(os.path.join(golden, "qgtc_attn_heads_abi.txt")).read().splitlines()


@pytest.mark.parametrize("heads", [1, 2])
def test_the_score_refuses_bad_arguments(lib, p, heads):
    big = 1 << 16

    def f(rp=p, kq=p, tl=p, T=2, n=100, A=p, B=p, ab=big, N=8, att=p, ae=8, slope=0.2, vp=p, vr=p, out=p, nv=9, heads=heads):
        return lib.qgtc_tiled_addscore_heads_f32(rp, kq, tl, T, n, A, B, ab, N, att, ae, slope, vp, vr, out, nv, heads, None)

    # invalid: the per-edge dot's list, then a missing att, the slope and the heads
    assert f(n=0) == EINVAL and f(n=(1 << 23) + 1) == EINVAL and f(N=0) == EINVAL and f(T=-1) == EINVAL
    for name in ("rp", "kq", "tl", "A", "B", "att", "vp", "vr", "out"):
        assert f(**{name: None}) == EINVAL, name
    assert f(nv=1 << 31) == EINVAL
    for slope in (-0.001, 1.001, 2.0, float("nan"), float("inf"), -float("inf")):
        assert f(slope=slope) == EINVAL, slope
    assert f(heads=0) == EINVAL and f(heads=-1) == EINVAL and f(heads=3) == EINVAL and f(N=9, heads=2) == EINVAL and f(heads=16) == EINVAL
    # misaligned
    assert f(tl=p + 4) == EALIGN
    for name in ("A", "B", "att", "out"):
        assert f(**{name: p + 2}) == EALIGN, name
    assert f(vp=p + 4) == EALIGN and f(vr=p + 1) == EALIGN
    # short: in elements n * N, and att in N
    assert f(ab=799) == ESIZE and f(ae=7) == ESIZE and f(n=1 << 23, ab=799) == ESIZE
    # the order: invalid before misaligned before short
    assert f(ab=799, A=p + 2) == EALIGN and f(ae=7, att=p + 2) == EALIGN and f(ab=799, B=None) == EINVAL
    assert f(A=p + 2, heads=0) == EINVAL and f(ab=799, heads=3) == EINVAL and f(vr=p + 1, heads=5) == EINVAL
    assert f(att=p + 2, slope=2.0) == EINVAL and f(ae=7, slope=float("nan")) == EINVAL and f(ae=7, att=None) == EINVAL
    assert f(ae=7, vp=p + 4) == EALIGN and f(ab=799, vr=None) == EINVAL
    # the slope's ends are in the domain: the next refusal is reached
    assert f(slope=0.0, ae=7) == ESIZE and f(slope=1.0, ae=7) == ESIZE
    # nothing to do: no device work
    assert f(T=0, rp=None, kq=None, tl=None, vp=None, vr=None) == OK and f(nv=0, out=None) == OK
    assert f(T=0, rp=None, kq=None, tl=None, vp=None, vr=None, heads=0) == EINVAL
    assert f(T=0, rp=None, kq=None, tl=None, vp=None, vr=None, att=None) == EINVAL


@pytest.mark.parametrize("heads", [1, 2])
@pytest.mark.parametrize("transposed", [False, True])
def test_the_gradients_refuse_bad_arguments(lib, p, transposed, heads):
    entry = lib.qgtc_tiled_addscore_grad_heads_f32_t if transposed else lib.qgtc_tiled_addscore_grad_heads_f32
    k = 4 if transposed else 3
    big = 1 << 16

    def f(idx=(p,) * k, T=2, n=100, own=p, nbr=p, xe=big, N=8, att=p, ae=8, slope=0.2, d_own=p, P=p, oe=big, vp=p, vr=p, g=p, nv=9,
          heads=heads):
        return entry(*idx, T, n, own, nbr, xe, N, att, ae, slope, d_own, P, oe, vp, vr, g, nv, heads, None)

    # invalid: the weighted sum's list (g in the place of the values), then att, the slope, the outputs and the heads
    assert f(n=0) == EINVAL and f(n=(1 << 23) + 1) == EINVAL and f(N=0) == EINVAL and f(T=-1) == EINVAL
    for name in ("own", "nbr", "att", "vp", "vr", "g"):
        assert f(**{name: None}) == EINVAL, name
    for i in range(k):
        assert f(idx=tuple(None if j == i else p for j in range(k))) == EINVAL
    assert f(d_own=None, P=None) == EINVAL
    assert f(nv=1 << 31) == EINVAL
    for slope in (-0.001, 1.001, float("nan"), float("inf")):
        assert f(slope=slope) == EINVAL, slope
    assert f(heads=0) == EINVAL and f(heads=-2) == EINVAL and f(heads=3) == EINVAL and f(N=9, heads=2) == EINVAL
    # misaligned
    assert f(idx=(p,) * (k - 1) + (p + 4,)) == EALIGN     # tiles off 16 bytes
    for name in ("own", "nbr", "att", "d_own", "P", "g"):
        assert f(**{name: p + 2}) == EALIGN, name
    assert f(d_own=None, P=p + 2) == EALIGN and f(d_own=p + 2, P=None) == EALIGN
    assert f(vp=p + 4) == EALIGN and f(vr=p + 1) == EALIGN
    # short
    assert f(xe=799) == ESIZE and f(oe=799) == ESIZE and f(ae=7) == ESIZE
    assert f(d_own=None, oe=799) == ESIZE and f(P=None, oe=799) == ESIZE
    # the order
    assert f(xe=799, g=None) == EINVAL and f(xe=799, vp=p + 4) == EALIGN and f(own=p + 2, vr=None) == EINVAL
    assert f(ae=7, nbr=p + 2) == EALIGN and f(xe=799, att=p + 2) == EALIGN and f(nbr=p + 2, slope=2.0) == EINVAL
    assert f(oe=799, d_own=None, P=None) == EINVAL and f(P=p + 2, att=None) == EINVAL
    assert f(xe=799, heads=0) == EINVAL and f(own=p + 2, heads=3) == EINVAL and f(N=0, heads=0) == EINVAL
    assert f(slope=0.0, ae=7) == ESIZE and f(slope=1.0, xe=799) == ESIZE
    # an adjacency without tiles is still checked
    none = dict(idx=(None,) * k, T=0, vp=None, vr=None, g=None)
    assert f(**none, att=None) == EINVAL and f(**none, d_own=None, P=None) == EINVAL and f(**none, heads=0) == EINVAL
    assert f(**none, own=p + 2) == EALIGN and f(**none, oe=799) == ESIZE
