"""C-ABI of the extremum tiled products (include/qgtc.h, "Extremum tiled products": qgtc_tiledmax_f32 / _t and qgtc_tiledsel_f32 / _t):
the four symbols are exported, the ABI version stays 11, and bad arguments are refused before any device work (no GPU needed).
The signatures come from the header (cabi.load())."""
import ctypes

import pytest

OK, EINVAL, ESIZE, EALIGN = 0, 1, 2, 3


@pytest.fixture(scope="module")
def lib():
    from qgtc_ppopp22_amd import cabi

    return cabi.load()


def _buf(words):
    b = (ctypes.c_uint32 * (words + 64))()
    addr = ctypes.addressof(b)
    return b, (addr + 255) & ~255   # keep the buffer alive; 256-byte aligned address inside it


def test_symbols_and_version(lib):
    assert lib.qgtc_tiledmax_f32 and lib.qgtc_tiledmax_f32_t and lib.qgtc_tiledsel_f32 and lib.qgtc_tiledsel_f32_t
    assert lib.qgtc_abi_version() == 11


@pytest.mark.parametrize("select", [False, True])
@pytest.mark.parametrize("transposed", [False, True])
def test_extremum_entries_refuse_bad_arguments(lib, transposed, select):
    keep, p = _buf(1 << 16)
    big = 1 << 16
    entry = getattr(lib, ("qgtc_tiledsel_f32" if select else "qgtc_tiledmax_f32") + ("_t" if transposed else ""))

    def fn(idx, T, n, N, x_elems=big, out_elems=big, arg_elems=big, X=p, out=p, arg=p, op=0):
        """idx: the index pointers and the tile words (3 on the row view, 4 on the column view)"""
        if select:
            return entry(*idx, T, n, X, x_elems, N, arg, arg_elems, out, out_elems, None)
        return entry(*idx, T, n, X, x_elems, N, op, out, out_elems, arg, arg_elems, None)

    ok = (p,) * (4 if transposed else 3)
    # ---- the refusals of the float products ----
    assert fn(ok, 1, 0, 8) == EINVAL                          # n < 1
    assert fn(ok, 1, -5, 8) == EINVAL
    assert fn(ok, 1, (1 << 23) + 1, 8) == EINVAL              # n > 2^23
    assert fn(ok, 1, 100, 0) == EINVAL                        # N < 1
    assert fn(ok, 1, 100, -3) == EINVAL
    assert fn(ok, -1, 100, 8) == EINVAL                       # negative n_tiles
    for k in range(len(ok)):                                  # tiles without one of the index arrays or the tile words
        assert fn(ok[:k] + (None,) + ok[k + 1:], 1, 100, 8) == EINVAL, k
    assert fn(ok, 1, 100, 8, X=None) == EINVAL                # no X / dY
    assert fn(ok, 1, 100, 8, out=None) == EINVAL              # no out
    assert fn((None,) * len(ok), 0, 100, 8, X=None) == EINVAL     # ... also without tiles
    assert fn((None,) * len(ok), 0, 100, 8, out=None) == EINVAL
    assert fn(ok, 1, 100, 8, x_elems=799) == ESIZE            # one float short of 100 x 8
    assert fn(ok, 1, 100, 8, out_elems=799) == ESIZE
    assert fn(ok, 1, 1 << 23, 1 << 20, x_elems=(1 << 43) - 1, out_elems=1 << 43, arg_elems=1 << 43) == ESIZE   # n * N does not wrap
    assert fn(ok[:-1] + (p + 4,), 1, 100, 8) == EALIGN        # tiles off a 16-byte boundary
    assert fn(ok[:-1] + (p + 8,), 1, 100, 8) == EALIGN
    for off in (1, 2, 3):
        assert fn(ok, 1, 100, 8, X=p + off) == EALIGN         # X / dY off a 4-byte boundary
        assert fn(ok, 1, 100, 8, out=p + off) == EALIGN       # out off a 4-byte boundary
    # ---- what the extremum entries add ----
    for off in (1, 2, 3):
        assert fn(ok, 1, 100, 8, arg=p + off) == EALIGN       # arg off a 4-byte boundary
    assert fn(ok, 1, 100, 8, arg_elems=799) == ESIZE          # arg one element short
    assert fn(ok, 1, 1 << 23, 1 << 20, x_elems=1 << 43, out_elems=1 << 43, arg_elems=(1 << 43) - 1) == ESIZE
    if select:
        assert fn(ok, 1, 100, 8, arg=None) == EINVAL          # the select reads arg
        assert fn((None,) * len(ok), 0, 100, 8, arg=None) == EINVAL
    else:
        for op in (-1, 2, 7):
            assert fn(ok, 1, 100, 8, op=op) == EINVAL         # op outside {0, 1}
            assert fn((None,) * len(ok), 0, 100, 8, op=op) == EINVAL
        assert fn(ok, 1, 100, 8, arg=None, arg_elems=0, x_elems=799) == ESIZE   # arg may be NULL: the other checks still run
        assert fn(ok, 1, 100, 8, arg=None, arg_elems=0, op=2) == EINVAL
