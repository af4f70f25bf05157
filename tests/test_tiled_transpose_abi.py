"""C-ABI of the transposed tiled adjacency (include/qgtc.h, "Transposed tiled adjacency": qgtc_tiled_colindex*, qgtc_tiledmm2*_t): bad
arguments are refused before any device work (no GPU needed), and the work-size query keeps to its domain.
The signatures come from the header (cabi.load()); test_abi_symbols checks that they are exported."""
import ctypes

import pytest

EINVAL, ESIZE, EALIGN, ENODEVICE = 1, 2, 3, 5


@pytest.fixture(scope="module")
def lib():
    from qgtc_ppopp22_amd import cabi

    return cabi.load()


def _buf(words):
    b = (ctypes.c_uint32 * (words + 64))()
    addr = ctypes.addressof(b)
    return b, (addr + 255) & ~255   # keep the buffer alive; 256-byte aligned address inside it


def test_work_words_domain(lib):
    assert lib.qgtc_tiled_colindex_work_words(0) == 0
    assert lib.qgtc_tiled_colindex_work_words(-1) == 0
    assert lib.qgtc_tiled_colindex_work_words(-(1 << 40)) == 0
    assert lib.qgtc_tiled_colindex_work_words((1 << 40) + 1) == 0
    # the query asks rocPRIM, which may need the current device: 0 where it fails, else at least the two key arrays (64-bit keys)
    for t in (1, 1000, 123457):
        w = lib.qgtc_tiled_colindex_work_words(t)
        assert w == 0 or w >= 4 * t


def test_colindex_refuses_bad_arguments(lib):
    keep, p = _buf(1 << 12)
    call = lib.qgtc_tiled_colindex
    assert call(p, p, 10, 0, p, p, p, p, 1 << 12, None) == EINVAL              # n < 1
    assert call(p, p, 10, (1 << 23) + 1, p, p, p, p, 1 << 12, None) == EINVAL  # n > 2^23
    assert call(p, p, -1, 100, p, p, p, p, 1 << 12, None) == EINVAL            # negative n_tiles
    assert call(p, p, 10, 100, None, p, p, p, 1 << 12, None) == EINVAL         # no col_ptr
    assert call(p, p, 0, 0, None, None, None, None, 0, None) == EINVAL         # n < 1 without tiles
    assert call(None, p, 10, 100, p, p, p, p, 1 << 12, None) == EINVAL         # tiles without row_ptr
    assert call(p, None, 10, 100, p, p, p, p, 1 << 12, None) == EINVAL         # tiles without kquad
    assert call(p, p, 10, 100, p, None, p, p, 1 << 12, None) == EINVAL         # tiles without col_tile
    assert call(p, p, 10, 100, p, p, None, p, 1 << 12, None) == EINVAL         # tiles without col_rb
    assert call(p, p, 10, 100, p, p, p, None, 1 << 12, None) == EINVAL         # tiles without a work buffer
    # a short work buffer: ESIZE wherever the size query can be answered
    need = lib.qgtc_tiled_colindex_work_words(10)
    assert call(p, p, 10, 100, p, p, p, p, need - 1 if need else 0, None) == (ESIZE if need else ENODEVICE)
    assert call(p, p, 10, 100, p, p, p, p, 0, None) == (ESIZE if need else ENODEVICE)


@pytest.mark.parametrize("which", ["bit", "int"])
def test_products_refuse_bad_arguments(lib, which):
    keep, p = _buf(1 << 16)
    big = 1 << 16
    if which == "bit":
        fn = lambda cp, ct, cr, tw, T, n, N, w, ob=2, out_words=big: lib.qgtc_tiledmm2bit_t(  # noqa: E731
            cp, ct, cr, tw, T, n, p, big, N, w, ob, p, out_words, None)
    else:
        fn = lambda cp, ct, cr, tw, T, n, N, w, ob=None, out_words=big: lib.qgtc_tiledmm2int_t(  # noqa: E731
            cp, ct, cr, tw, T, n, p, big, N, w, p, out_words, None)
    assert fn(p, p, p, p, 1, 0, 8, 2) == EINVAL                 # n < 1
    assert fn(p, p, p, p, 1, (1 << 23) + 1, 8, 2) == EINVAL     # n > 2^23
    assert fn(p, p, p, p, 1, 100, 0, 2) == EINVAL               # N < 1
    assert fn(p, p, p, p, 1, 100, 8, 0) == EINVAL               # bit2 < 1
    assert fn(p, p, p, p, 1, 100, 8, 9) == EINVAL               # bit2 > 8
    assert fn(p, p, p, p, -1, 100, 8, 2) == EINVAL              # negative n_tiles
    assert fn(None, p, p, p, 1, 100, 8, 2) == EINVAL            # no col_ptr
    assert fn(p, None, p, p, 1, 100, 8, 2) == EINVAL            # tiles without col_tile
    assert fn(p, p, None, p, 1, 100, 8, 2) == EINVAL            # tiles without col_rb
    assert fn(p, p, p, None, 1, 100, 8, 2) == EINVAL            # tiles without tile words
    if which == "bit":
        assert fn(p, p, p, p, 1, 100, 8, 2, ob=33) == EINVAL    # output_bit > 32
        assert fn(p, p, p, p, 1, 100, 8, 2, ob=0) == EINVAL     # output_bit < 1
        assert fn(p, p, p, p, 1, 100, 8, 2, ob=4, out_words=4 * 104 * 4 - 1) == ESIZE   # one word short of 4 planes x 104 rows
    else:
        assert fn(p, p, p, p, 1, 100, 8, 2, out_words=799) == ESIZE                     # one float short of 100 x 8
    # the C-ABI mirrors of the forward entries refuse the same way (the transposed entries add no domain of their own)
    assert lib.qgtc_tiledmm2bit_t(p, p, p, p, 1, 100, None, big, 8, 2, 2, p, big, None) == EINVAL   # no X
    assert lib.qgtc_tiledmm2int_t(p, p, p, p, 1, 100, p, big, 8, 2, None, big, None) == EINVAL      # no out


@pytest.mark.parametrize("which", ["bit", "int"])
def test_products_need_col_ptr_and_keep_the_order_of_refusals(lib, which):
    """The bit kernels read col_ptr without looking at n_tiles, so the entries want it even for an adjacency without tiles; and of two
    faults the invalid argument is reported before the misaligned one, and either before the short output."""
    keep, p = _buf(1 << 16)
    big = 1 << 16

    def fn(cp=p, ct=p, cr=p, tl=p, T=1, X=p, w=2, ob=2, out_size=big):
        tail = (w, ob, p, out_size, None) if which == "bit" else (w, p, out_size, None)
        return getattr(lib, f"qgtc_tiledmm2{which}_t")(cp, ct, cr, tl, T, 100, X, big, 8, *tail)

    assert fn(cp=None, ct=None, cr=None, tl=None, T=0) == EINVAL   # no col_ptr, no tiles
    assert fn(cp=None, T=0) == EINVAL
    assert fn(w=9, out_size=10) == EINVAL                     # bit2 > 8 and a short output
    assert fn(X=p + 4, out_size=10) == EALIGN                 # X off a 16-byte boundary and a short output
    if which == "bit":
        assert fn(X=p + 4, ob=33) == EALIGN                   # the shared check (X misaligned) comes before the entry's own (output_bit)
