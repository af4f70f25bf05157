"""C-ABI of the edge values (include/qgtc.h, "Edge values": qgtc_tiled_value_index, qgtc_tiled_edge_slots, qgtc_tiled_edge_endpoints,
qgtc_tiledmm_f32_edge / _t_edge and qgtc_tiled_sddmm_f32): the six symbols are exported, the ABI version stays 11, and bad arguments
are refused before any device work, invalid before misaligned before short (no GPU needed). The signatures come from the header (cabi.load())."""
import ctypes
import os

import pytest

OK, EINVAL, ESIZE, EALIGN = 0, 1, 2, 3
NAMES = ("qgtc_tiled_value_index", "qgtc_tiled_edge_slots", "qgtc_tiled_edge_endpoints", "qgtc_tiledmm_f32_edge",
         "qgtc_tiledmm_f32_t_edge", "qgtc_tiled_sddmm_f32")


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
    assert "Edge values" in text
    for name in NAMES:
        assert f"int {name}(" in text, name
    assert "#define QGTC_ABI_VERSION 11" in text


def test_value_index_refuses_bad_arguments(lib, p):
    f = lib.qgtc_tiled_value_index
    assert f(p, -1, p, p, None) == EINVAL
    for bad in ((None, p, p), (p, None, p), (p, p, None)):
        assert f(bad[0], 3, bad[1], bad[2], None) == EINVAL
    assert f(p + 4, 3, p, p, None) == EALIGN      # tiles off 16 bytes
    assert f(p, 3, p + 4, p, None) == EALIGN      # counts off 8
    assert f(p, 3, p, p + 1, None) == EALIGN      # val_row off 2
    assert f(None, 0, None, None, None) == OK     # nothing to do, no device work


def test_edge_slots_refuses_bad_arguments(lib, p):
    def f(rp=p, kq=p, tl=p, T=2, n=100, vp=p, vr=p, src=p, dst=p, E=5, slot=p):
        return lib.qgtc_tiled_edge_slots(rp, kq, tl, T, n, vp, vr, src, dst, E, slot, None)

    assert f(n=0) == EINVAL and f(n=(1 << 23) + 1) == EINVAL and f(T=-1) == EINVAL
    for name in ("rp", "kq", "tl", "vp", "vr", "src", "dst", "slot"):
        assert f(**{name: None}) == EINVAL, name
    assert f(tl=p + 4) == EALIGN
    for name in ("vp", "src", "dst", "slot"):
        assert f(**{name: p + 4}) == EALIGN, name
    assert f(vr=p + 1) == EALIGN
    assert f(tl=p + 4, src=None) == EINVAL        # invalid before misaligned
    assert f(n=1 << 23, tl=p + 4) == EALIGN and f(n=1 << 23, slot=p + 4) == EALIGN   # n = 2^23 is in range: the next refusal is reached
    assert f(E=0, src=None, dst=None, slot=None) == OK


def test_edge_endpoints_refuses_bad_arguments(lib, p):
    def f(rp=p, kq=p, tl=p, T=2, n=100, vp=p, vr=p, row=p, col=p, nv=7):
        return lib.qgtc_tiled_edge_endpoints(rp, kq, tl, T, n, vp, vr, row, col, nv, None)

    assert f(n=0) == EINVAL and f(n=(1 << 23) + 1) == EINVAL and f(T=-1) == EINVAL
    for name in ("rp", "kq", "tl", "vp", "vr", "row", "col"):
        assert f(**{name: None}) == EINVAL, name
    assert f(nv=1 << 31) == EINVAL                # slots are 32-bit inside the kernels
    assert f(tl=p + 4) == EALIGN and f(vp=p + 4) == EALIGN and f(vr=p + 1) == EALIGN
    assert f(row=p + 2) == EALIGN and f(col=p + 2) == EALIGN
    assert f(T=0, nv=0, rp=None, kq=None, tl=None, vp=None, vr=None, row=None, col=None) == OK


@pytest.mark.parametrize("transposed", [False, True])
def test_weighted_products_refuse_bad_arguments(lib, p, transposed):
    entry = lib.qgtc_tiledmm_f32_t_edge if transposed else lib.qgtc_tiledmm_f32_edge
    k = 4 if transposed else 3
    big = 1 << 16

    def f(idx=(p,) * k, T=2, n=100, X=p, xe=big, N=8, rs=None, out=p, oe=big, vp=p, vr=p, vals=p, nv=9):
        return entry(*idx, T, n, X, xe, N, rs, out, oe, vp, vr, vals, nv, None)

    # the refusals of qgtc_tiledmm_f32, in its order
    assert f(n=0) == EINVAL and f(n=(1 << 23) + 1) == EINVAL and f(N=0) == EINVAL and f(T=-1) == EINVAL
    assert f(X=None) == EINVAL and f(out=None) == EINVAL
    for i in range(k):
        assert f(idx=tuple(None if j == i else p for j in range(k))) == EINVAL
    assert f(idx=(p,) * (k - 1) + (p + 4,)) == EALIGN     # tiles off 16 bytes
    assert f(X=p + 2) == EALIGN and f(out=p + 2) == EALIGN and f(rs=p + 2) == EALIGN
    assert f(xe=799) == ESIZE and f(oe=799) == ESIZE
    # the edge values' own
    for name in ("vp", "vr", "vals"):
        assert f(**{name: None}) == EINVAL, name
    assert f(nv=1 << 31) == EINVAL
    assert f(vp=p + 4) == EALIGN and f(vr=p + 1) == EALIGN and f(vals=p + 2) == EALIGN
    # invalid before misaligned before short, across the two lists
    assert f(xe=799, vals=None) == EINVAL
    assert f(xe=799, vp=p + 4) == EALIGN
    assert f(X=p + 2, vr=None) == EINVAL


def test_sddmm_refuses_bad_arguments(lib, p):
    big = 1 << 16

    def f(rp=p, kq=p, tl=p, T=2, n=100, A=p, B=p, ab=big, N=8, vp=p, vr=p, out=p, nv=9):
        return lib.qgtc_tiled_sddmm_f32(rp, kq, tl, T, n, A, B, ab, N, vp, vr, out, nv, None)

    assert f(n=0) == EINVAL and f(n=(1 << 23) + 1) == EINVAL and f(N=0) == EINVAL and f(T=-1) == EINVAL
    for name in ("rp", "kq", "tl", "A", "B", "vp", "vr", "out"):
        assert f(**{name: None}) == EINVAL, name
    assert f(nv=1 << 31) == EINVAL
    assert f(tl=p + 4) == EALIGN
    for name in ("A", "B", "out"):
        assert f(**{name: p + 2}) == EALIGN, name
    assert f(vp=p + 4) == EALIGN and f(vr=p + 1) == EALIGN
    assert f(ab=799) == ESIZE
    assert f(ab=799, A=p + 2) == EALIGN and f(ab=799, B=None) == EINVAL
    assert f(n=1 << 23, ab=799) == ESIZE          # n = 2^23 is in range: the next refusal is reached
    assert f(ab=799, tl=p + 4) == EALIGN          # misaligned tile words before short operands
