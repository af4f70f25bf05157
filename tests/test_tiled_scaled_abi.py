"""C-ABI of the scaled tiled products and the degrees (include/qgtc.h, "Scaled tiled products and degrees": qgtc_tiled_degrees,
qgtc_tiledmm2bit_scaled / _int_scaled / _bit_t_scaled / _int_t_scaled): bad arguments are refused before any device work (no GPU
needed). The signatures come from the header (cabi.load()); test_abi_symbols checks that they are exported."""
import ctypes

import pytest

EINVAL, ESIZE, EALIGN = 1, 2, 3


@pytest.fixture(scope="module")
def lib():
    from qgtc_ppopp22_amd import cabi

    return cabi.load()


def _buf(words):
    b = (ctypes.c_uint32 * (words + 64))()
    addr = ctypes.addressof(b)
    return b, (addr + 255) & ~255   # keep the buffer alive; 256-byte aligned address inside it


def test_degrees_refuse_bad_arguments(lib):
    keep, p = _buf(1 << 12)
    call = lib.qgtc_tiled_degrees
    assert call(p, p, p, 1, 0, p, p, p, p, None) == EINVAL                    # n < 1
    assert call(p, p, p, 1, (1 << 23) + 1, p, p, p, p, None) == EINVAL        # n > 2^23
    assert call(p, p, p, -1, 100, p, p, p, p, None) == EINVAL                 # negative n_tiles
    assert call(None, p, p, 1, 100, p, p, p, p, None) == EINVAL               # tiles without row_ptr
    assert call(p, None, p, 1, 100, p, p, p, p, None) == EINVAL               # tiles without kquad
    assert call(p, p, None, 1, 100, p, p, p, p, None) == EINVAL               # tiles without tile words
    assert call(p, p, p, 1, 100, None, None, None, None, None) == EINVAL      # all four outputs NULL
    assert call(None, None, None, 0, 100, None, None, None, None, None) == EINVAL   # the same without tiles
    assert call(p, p, p, 1, 100, None, p, p, None, None) == EINVAL            # out_inv without out_deg
    assert call(p, p, p, 1, 100, p, None, None, p, None) == EINVAL            # in_inv without in_deg
    assert call(p, p, p, 1, 100, None, None, p, p, None) == EINVAL            # reciprocals alone
    assert call(p, p, p + 4, 1, 100, p, p, p, p, None) == EALIGN              # tiles off a 16-byte boundary
    assert call(p, p, p + 4, 1, 1 << 23, p, p, p, p, None) == EALIGN          # n = 2^23 is in range: the next refusal is reached
    assert call(p, p, p + 4, 1, 100, None, None, p, p, None) == EINVAL        # invalid before misaligned


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("which", ["bit", "int"])
def test_scaled_products_refuse_bad_arguments(lib, which, transposed):
    keep, p = _buf(1 << 16)
    big = 1 << 16
    name = f"qgtc_tiledmm2{which}{'_t' if transposed else ''}_scaled"
    entry = getattr(lib, name)

    def fn(idx, T, n, N, w, ob=2, out_words=big, X=p, scale=p, out=p):
        """idx: the index pointers and the tile words (3 forward: row_ptr, kquad, tiles; 4 transposed: col_ptr, col_tile, col_rb, tiles)"""
        args = list(idx) + [T, n, X, big, N, w] + ([ob] if which == "bit" else []) + [scale, out, out_words, None]
        return entry(*args)

    ok = (p,) * (4 if transposed else 3)
    assert fn(ok, 1, 0, 8, 2) == EINVAL                       # n < 1
    assert fn(ok, 1, (1 << 23) + 1, 8, 2) == EINVAL           # n > 2^23
    assert fn(ok, 1, 100, 0, 2) == EINVAL                     # N < 1
    assert fn(ok, 1, 100, 8, 0) == EINVAL                     # bit2 < 1
    assert fn(ok, 1, 100, 8, 9) == EINVAL                     # bit2 > 8
    assert fn(ok, -1, 100, 8, 2) == EINVAL                    # negative n_tiles
    assert fn((None,) + ok[1:], 1, 100, 8, 2) == EINVAL       # no row_ptr / col_ptr
    for k in range(1, len(ok)):                               # tiles without kquad / col_tile / col_rb / tile words
        assert fn(ok[:k] + (None,) + ok[k + 1:], 1, 100, 8, 2) == EINVAL, k
    assert fn(ok, 1, 100, 8, 2, X=None) == EINVAL             # no X
    assert fn(ok, 1, 100, 8, 2, out=None) == EINVAL           # no out
    assert fn(ok, 1, 100, 8, 2, scale=None) == EINVAL         # no row_scale
    assert fn((p,) + (None,) * (len(ok) - 1), 0, 100, 8, 2, scale=None) == EINVAL   # ... also without tiles
    assert fn(ok, 1, 100, 8, 2, X=p + 4) == EALIGN            # X off a 16-byte boundary
    assert fn(ok, 1, 100, 8, 2, out=p + 4) == EALIGN          # out off a 16-byte boundary
    assert fn(ok[:-1] + (p + 4,), 1, 100, 8, 2) == EALIGN     # tiles off a 16-byte boundary
    if which == "bit":
        assert fn(ok, 1, 100, 8, 2, ob=33) == EINVAL          # output_bit > 32
        assert fn(ok, 1, 100, 8, 2, ob=0) == EINVAL           # output_bit < 1
        assert fn(ok, 1, 100, 8, 2, ob=4, out_words=4 * 104 * 4 - 1) == ESIZE   # one word short of 4 planes x 104 rows
    else:
        assert fn(ok, 1, 100, 8, 2, out_words=799) == ESIZE   # one float short of 100 x 8
    # the bit kernels read row_ptr / col_ptr without looking at n_tiles: wanted even for an adjacency without tiles
    assert fn((None,) * len(ok), 0, 100, 8, 2) == EINVAL
    assert fn((None,) + ok[1:], 0, 100, 8, 2) == EINVAL
    # two faults at once: the shared check (invalid, then misaligned) before the entry's own (row_scale, output_bit), and the short output last
    assert fn(ok, 1, 100, 8, 2, X=p + 4, scale=None) == EALIGN
    assert fn(ok, 1, 100, 8, 9, out_words=10) == EINVAL
    assert fn(ok, 1, 100, 8, 2, scale=None, out_words=10) == EINVAL
    if which == "bit":
        assert fn(ok, 1, 100, 8, 2, X=p + 4, ob=33) == EALIGN
