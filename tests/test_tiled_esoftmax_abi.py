"""C-ABI of the edge softmax (include/qgtc.h, "Edge softmax": qgtc_tiled_edge_softmax_f32 / _t and qgtc_tiled_edge_softmax_grad_f32 /
_t): the four symbols are exported and declared, the ABI version stays 11, and bad arguments are refused before any device work,
invalid before misaligned (no GPU needed). The signatures come from the header (cabi.load())."""
import ctypes
import os

import pytest

OK, EINVAL, ESIZE, EALIGN = 0, 1, 2, 3
NAMES = ("qgtc_tiled_edge_softmax_f32", "qgtc_tiled_edge_softmax_f32_t", "qgtc_tiled_edge_softmax_grad_f32",
         "qgtc_tiled_edge_softmax_grad_f32_t")


@pytest.fixture(scope="module")
def lib():
    from qgtc_ppopp22_amd import cabi

    return cabi.load()


@pytest.fixture(scope="module")
def p():
    b = (ctypes.c_uint32 * ((1 << 16) + 64))()
    addr = (ctypes.addressof(b) + 255) & ~255   # 256-byte aligned address inside the buffer
    yield addr
    del b


def test_symbols_and_version(lib):
    for name in NAMES:
        assert getattr(lib, name), name
    assert lib.qgtc_abi_version() == 11


def test_the_header_declares_the_entries():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qgtc.h")).read()
    assert "Edge softmax" in text
    for name in NAMES:
        assert f"int {name}(" in text, name
    assert "#define QGTC_ABI_VERSION 11" in text


@pytest.mark.parametrize("transposed", [False, True])
def test_forward_refuses_bad_arguments(lib, p, transposed):
    entry = lib.qgtc_tiled_edge_softmax_f32_t if transposed else lib.qgtc_tiled_edge_softmax_f32
    k = 4 if transposed else 3   # the view's index arrays, then tiles

    def f(idx=(p,) * k, T=2, n=100, vp=p, vr=p, logits=p, alpha=p, nv=9, m=p, inv=p):
        return entry(*idx, T, n, vp, vr, logits, alpha, nv, m, inv, None)

    assert f(n=0) == EINVAL and f(n=(1 << 23) + 1) == EINVAL and f(T=-1) == EINVAL
    for i in range(k):
        assert f(idx=tuple(None if j == i else p for j in range(k))) == EINVAL, i
    for name in ("vp", "vr", "logits", "alpha"):
        assert f(**{name: None}) == EINVAL, name
    assert f(nv=1 << 31) == EINVAL                          # slots are 32-bit inside the kernels
    assert f(idx=(p,) * (k - 1) + (p + 4,)) == EALIGN       # tiles off 16 bytes
    assert f(vp=p + 4) == EALIGN and f(vr=p + 1) == EALIGN
    for name in ("logits", "alpha", "m", "inv"):
        assert f(**{name: p + 2}) == EALIGN, name
    # invalid before misaligned, across the two lists
    assert f(logits=p + 2, vr=None) == EINVAL and f(vp=p + 4, alpha=None) == EINVAL and f(n=0, m=p + 2) == EINVAL
    assert f(idx=(p,) * (k - 1) + (p + 4,), nv=1 << 31) == EINVAL
    assert f(n=1 << 23, vr=p + 1) == EALIGN                 # n = 2^23 is in range: the next refusal is reached
    # nothing to do, no device work: m and inv not wanted
    assert f(idx=(None,) * k, T=0, vp=None, vr=None, logits=None, alpha=None, nv=0, m=None, inv=None) == OK
    assert f(idx=(None,) * k, T=0, vp=None, vr=None, nv=0, m=None, inv=None) == OK
    assert f(nv=0, logits=None, alpha=None, m=None, inv=None) == OK


@pytest.mark.parametrize("transposed", [False, True])
def test_gradient_refuses_bad_arguments(lib, p, transposed):
    entry = lib.qgtc_tiled_edge_softmax_grad_f32_t if transposed else lib.qgtc_tiled_edge_softmax_grad_f32
    k = 4 if transposed else 3

    def f(idx=(p,) * k, T=2, n=100, vp=p, vr=p, alpha=p, g=p, out=p, nv=9):
        return entry(*idx, T, n, vp, vr, alpha, g, out, nv, None)

    assert f(n=0) == EINVAL and f(n=(1 << 23) + 1) == EINVAL and f(T=-1) == EINVAL
    for i in range(k):
        assert f(idx=tuple(None if j == i else p for j in range(k))) == EINVAL, i
    for name in ("vp", "vr", "alpha", "g", "out"):
        assert f(**{name: None}) == EINVAL, name
    assert f(nv=1 << 31) == EINVAL
    assert f(idx=(p,) * (k - 1) + (p + 4,)) == EALIGN
    assert f(vp=p + 4) == EALIGN and f(vr=p + 1) == EALIGN
    for name in ("alpha", "g", "out"):
        assert f(**{name: p + 2}) == EALIGN, name
    assert f(g=p + 2, vp=None) == EINVAL and f(vr=p + 1, out=None) == EINVAL
    assert f(idx=(None,) * k, T=0, vp=None, vr=None, alpha=None, g=None, out=None, nv=0) == OK
    assert f(nv=0, alpha=None, g=None, out=None) == OK
