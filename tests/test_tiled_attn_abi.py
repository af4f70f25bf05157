"""C-ABI of the attention tiled products (include/qgtc.h, "Attention tiled products": qgtc_tiledatt_f32 / _t, qgtc_tiledatt_grad_f32 / _t
and qgtc_rowdot_f32): the five symbols are exported, the ABI version stays 11, and bad arguments are refused before any device work
(no GPU needed). The signatures come from the header (cabi.load())."""
import ctypes

import pytest

OK, EINVAL, ESIZE, EALIGN = 0, 1, 2, 3
NAMES = ("qgtc_tiledatt_f32", "qgtc_tiledatt_f32_t", "qgtc_tiledatt_grad_f32", "qgtc_tiledatt_grad_f32_t", "qgtc_rowdot_f32")


@pytest.fixture(scope="module")
def lib():
    from qgtc_ppopp22_amd import cabi

    return cabi.load()


def _buf(words):
    b = (ctypes.c_uint32 * (words + 64))()
    addr = ctypes.addressof(b)
    return b, (addr + 255) & ~255   # keep the buffer alive; 256-byte aligned address inside it


def test_symbols_and_version(lib):
    for name in NAMES:
        assert getattr(lib, name), name
    assert lib.qgtc_abi_version() == 11


def test_the_header_declares_the_entries():
    import os

    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qgtc.h")).read()
    assert "Attention tiled products" in text
    for name in NAMES:
        assert f"int {name}(" in text, name
    assert "#define QGTC_ABI_VERSION 11" in text


@pytest.mark.parametrize("grad", [False, True])
@pytest.mark.parametrize("transposed", [False, True])
def test_attention_entries_refuse_bad_arguments(lib, transposed, grad):
    keep, p = _buf(1 << 16)
    big = 1 << 16
    entry = getattr(lib, ("qgtc_tiledatt_grad_f32" if grad else "qgtc_tiledatt_f32") + ("_t" if transposed else ""))
    vectors = ("own", "nbr", "m", "inv", "D") if grad else ("own", "nbr", "shift", "m", "inv")

    def fn(idx, T, n, N, x_elems=big, out_elems=big, X=p, out=p, other=p, slope=0.2, flag=0, **vec):
        """idx: the index pointers and the tile words (3 on the row view, 4 on the column view); vec: the per-node vectors"""
        v = {name: vec.pop(name, p) for name in vectors}
        assert not vec, vec
        if grad:
            return entry(*idx, T, n, X, other, x_elems, N, v["own"], v["nbr"], slope, flag, v["m"], v["inv"], v["D"], out, out_elems, None)
        return entry(*idx, T, n, X, x_elems, N, v["own"], v["nbr"], slope, flag, v["shift"], v["m"], v["inv"], out, out_elems, None)

    ok = (p,) * (4 if transposed else 3)
    none = (None,) * len(ok)
    # ---- the refusals of the float products ----
    assert fn(ok, 1, 0, 8) == EINVAL                          # n < 1
    assert fn(ok, 1, -5, 8) == EINVAL
    assert fn(ok, 1, (1 << 23) + 1, 8) == EINVAL              # n > 2^23
    assert fn(ok, 1, 100, 0) == EINVAL                        # N < 1
    assert fn(ok, 1, 100, -3) == EINVAL
    assert fn(ok, -1, 100, 8) == EINVAL                       # negative n_tiles
    for k in range(len(ok)):                                  # tiles without one of the index arrays or the tile words
        assert fn(ok[:k] + (None,) + ok[k + 1:], 1, 100, 8) == EINVAL, k
    assert fn(ok, 1, 100, 8, X=None) == EINVAL                # no X / A
    assert fn(ok, 1, 100, 8, out=None) == EINVAL              # no out
    assert fn(none, 0, 100, 8, X=None) == EINVAL              # ... also without tiles
    assert fn(none, 0, 100, 8, out=None) == EINVAL
    assert fn(ok, 1, 100, 8, x_elems=799) == ESIZE            # one float short of 100 x 8
    assert fn(ok, 1, 100, 8, out_elems=99 if grad else 799) == ESIZE
    assert fn(ok, 1, 1 << 23, 1 << 20, x_elems=(1 << 43) - 1, out_elems=1 << 43) == ESIZE     # n * N does not wrap
    assert fn(ok[:-1] + (p + 4,), 1, 100, 8) == EALIGN        # tiles off a 16-byte boundary
    assert fn(ok[:-1] + (p + 8,), 1, 100, 8) == EALIGN
    assert fn(ok[:-1] + (p + 4,), 1, 100, 8, out_elems=99 if grad else 799) == EALIGN   # ... before a short output
    for off in (1, 2, 3):
        assert fn(ok, 1, 100, 8, X=p + off) == EALIGN         # X / A off a 4-byte boundary
        assert fn(ok, 1, 100, 8, out=p + off) == EALIGN       # out off a 4-byte boundary
    # ---- what the attention entries add ----
    for slope in (-0.001, 1.001, 2.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert fn(ok, 1, 100, 8, slope=slope) == EINVAL       # a slope outside [0, 1]
        assert fn(none, 0, 100, 8, slope=slope) == EINVAL
    for flag in (-1, 2, 7):
        assert fn(ok, 1, 100, 8, flag=flag) == EINVAL         # backward / nbr_owns outside {0, 1}
    for flag in (0, 1):
        for name in vectors:
            if not grad and name == "m" and flag == 1:
                continue                                      # the backward mode does not touch m
            assert fn(ok, 1, 100, 8, flag=flag, **{name: None}) == EINVAL, (name, flag)
            assert fn(none, 0, 100, 8, flag=flag, **{name: None}) == EINVAL, (name, flag)
            for off in (1, 2, 3):
                assert fn(ok, 1, 100, 8, flag=flag, **{name: p + off}) == EALIGN, (name, flag)
        assert fn(ok, 1, 100, 8, flag=flag, x_elems=799) == ESIZE
    if grad:
        assert fn(ok, 1, 100, 8, other=None) == EINVAL        # the neighbours' matrix
        for off in (1, 2, 3):
            assert fn(ok, 1, 100, 8, other=p + off) == EALIGN
        assert fn(ok, 1, 100, 8, out_elems=100, x_elems=799) == ESIZE
    # invalid beats misaligned beats short, as for the float products
    assert fn(ok, 1, 100, 8, X=p + 1, slope=2.0, x_elems=1) == EINVAL
    assert fn(ok, 1, 100, 8, X=p + 1, x_elems=1) == EALIGN


def test_rowdot_refuses_bad_arguments(lib):
    keep, p = _buf(1 << 16)
    big = 1 << 16

    def fn(n, N, A=p, B=p, out=p, ab_elems=big, out_elems=big):
        return lib.qgtc_rowdot_f32(A, B, ab_elems, n, N, out, out_elems, None)

    for n, N in ((0, 8), (-1, 8), ((1 << 23) + 1, 8), (100, 0), (100, -2)):
        assert fn(n, N) == EINVAL
    for name in ("A", "B", "out"):
        assert fn(100, 8, **{name: None}) == EINVAL
        for off in (1, 2, 3):
            assert fn(100, 8, **{name: p + off}) == EALIGN
    assert fn(100, 8, ab_elems=799) == ESIZE
    assert fn(100, 8, out_elems=99) == ESIZE
    assert fn(1 << 23, 1 << 20, ab_elems=(1 << 43) - 1, out_elems=1 << 43) == ESIZE
