"""C-ABI of the float tiled products (include/qgtc.h, "Float tiled products": qgtc_tiledmm_f32 / qgtc_tiledmm_f32_t): both symbols are
exported, the ABI version stays 11, and bad arguments are refused before any device work (no GPU needed).
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
    assert lib.qgtc_tiledmm_f32 and lib.qgtc_tiledmm_f32_t
    assert lib.qgtc_abi_version() == 11


@pytest.mark.parametrize("transposed", [False, True])
def test_float_products_refuse_bad_arguments(lib, transposed):
    keep, p = _buf(1 << 16)
    big = 1 << 16
    entry = lib.qgtc_tiledmm_f32_t if transposed else lib.qgtc_tiledmm_f32

    def fn(idx, T, n, N, x_elems=big, out_elems=big, X=p, scale=p, out=p):
        """idx: the index pointers and the tile words (3 forward: row_ptr, kquad, tiles; 4 transposed: col_ptr, col_tile, col_rb, tiles)"""
        return entry(*idx, T, n, X, x_elems, N, scale, out, out_elems, None)

    ok = (p,) * (4 if transposed else 3)
    assert fn(ok, 1, 0, 8) == EINVAL                          # n < 1
    assert fn(ok, 1, -5, 8) == EINVAL
    assert fn(ok, 1, (1 << 23) + 1, 8) == EINVAL              # n > 2^23
    assert fn(ok, 1, 100, 0) == EINVAL                        # N < 1
    assert fn(ok, 1, 100, -3) == EINVAL
    assert fn(ok, -1, 100, 8) == EINVAL                       # negative n_tiles
    for k in range(len(ok)):                                  # tiles without row_ptr / kquad / col_ptr / col_tile / col_rb / tile words
        assert fn(ok[:k] + (None,) + ok[k + 1:], 1, 100, 8) == EINVAL, k
    assert fn(ok, 1, 100, 8, X=None) == EINVAL                # no X
    assert fn(ok, 1, 100, 8, out=None) == EINVAL              # no out
    assert fn((None,) * len(ok), 0, 100, 8, X=None) == EINVAL     # ... also without tiles
    assert fn((None,) * len(ok), 0, 100, 8, out=None) == EINVAL
    assert fn(ok, 1, 100, 8, x_elems=799) == ESIZE            # one float short of 100 x 8
    assert fn(ok, 1, 100, 8, out_elems=799) == ESIZE
    assert fn(ok, 1, 100, 8, scale=None, out_elems=799) == ESIZE
    assert fn(ok, 1, 1 << 23, 1 << 20, x_elems=(1 << 43) - 1, out_elems=1 << 43) == ESIZE   # n * N does not wrap in 32 bits
    assert fn(ok[:-1] + (p + 4,), 1, 100, 8) == EALIGN        # tiles off a 16-byte boundary
    assert fn(ok[:-1] + (p + 8,), 1, 100, 8) == EALIGN
    assert fn(ok[:-1] + (p + 4,), 1, 100, 8, out_elems=799) == EALIGN   # ... before a short output
    for off in (1, 2, 3):
        assert fn(ok, 1, 100, 8, X=p + off) == EALIGN         # X off a 4-byte boundary
        assert fn(ok, 1, 100, 8, out=p + off) == EALIGN       # out off a 4-byte boundary
        assert fn(ok, 1, 100, 8, scale=p + off) == EALIGN     # row_scale off a 4-byte boundary
