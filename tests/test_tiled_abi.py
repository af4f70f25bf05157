"""C-ABI of the tile-compressed adjacency (include/qgtc.h, qgtc_tiled_*): exported, and bad arguments are refused before any device
work (no GPU needed). The signatures come from the header (cabi.load())."""
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


def test_entries_are_exported(lib):
    for name in ("qgtc_tiled_work_words", "qgtc_tiled_count", "qgtc_tiled_fill", "qgtc_tiledmm2bit", "qgtc_tiledmm2int"):
        assert hasattr(lib, name)
    assert lib.qgtc_tiled_work_words(0) == 0


def test_count_and_fill_refuse_bad_arguments(lib):
    keep, p = _buf(1024)
    assert lib.qgtc_tiled_count(p, p, 10, 0, p, p, 1024, None, None) == EINVAL            # n < 1
    assert lib.qgtc_tiled_count(p, p, 10, (1 << 23) + 1, p, p, 1024, None, None) == EINVAL  # n > 2^23
    assert lib.qgtc_tiled_count(None, p, 10, 100, p, p, 1024, None, None) == EINVAL       # edges without src
    assert lib.qgtc_tiled_count(p, p, 10, 100, None, p, 1024, None, None) == EINVAL       # no row_ptr
    assert lib.qgtc_tiled_count(p, p, 10, 100, p, None, 0, None, None) == EINVAL          # edges without a work buffer
    assert lib.qgtc_tiled_fill(10, 100, -1, p, p, p, 1024, None) == EINVAL                # negative tile count
    assert lib.qgtc_tiled_fill(10, 100, 11, p, p, p, 1024, None) == EINVAL                # more tiles than edges
    assert lib.qgtc_tiled_fill(10, 100, 3, None, p, p, 1024, None) == EINVAL              # no kquad


def test_products_refuse_bad_arguments(lib):
    keep, p = _buf(1 << 16)
    for fn, tail in ((lib.qgtc_tiledmm2bit, lambda w, ob: (w, ob, p, 1 << 16, None)), (lib.qgtc_tiledmm2int, lambda w, ob: (w, p, 1 << 16, None))):
        assert fn(p, p, p, 1, 0, p, 1 << 16, 8, *tail(2, 2)) == EINVAL       # n < 1
        assert fn(p, p, p, 1, 100, p, 1 << 16, 0, *tail(2, 2)) == EINVAL     # N < 1
        assert fn(p, p, p, 1, 100, p, 1 << 16, 8, *tail(9, 2)) == EINVAL     # bit2 > 8
        assert fn(p, p, p, 1, 100, p, 1 << 16, 8, *tail(0, 2)) == EINVAL     # bit2 < 1
        assert fn(p, None, p, 1, 100, p, 1 << 16, 8, *tail(2, 2)) == EINVAL  # tiles without kquad
        assert fn(None, p, p, 1, 100, p, 1 << 16, 8, *tail(2, 2)) == EINVAL  # no row_ptr
    assert lib.qgtc_tiledmm2bit(p, p, p, 1, 100, p, 1 << 16, 8, 2, 33, p, 1 << 16, None) == EINVAL   # output_bit > 32
    assert lib.qgtc_tiledmm2bit(p, p, p, 1, 100, p, 1 << 16, 8, 2, 4, p, 10, None) == ESIZE          # out too small
    assert lib.qgtc_tiledmm2int(p, p, p, 1, 100, p, 1 << 16, 8, 2, p, 799, None) == ESIZE            # out too small


@pytest.mark.parametrize("which", ["bit", "int"])
def test_products_need_row_ptr_and_keep_the_order_of_refusals(lib, which):
    """The bit kernels read row_ptr without looking at n_tiles, so the entries want it even for an adjacency without tiles; and of two
    faults the invalid argument is reported before the misaligned one, and either before the short output."""
    keep, p = _buf(1 << 16)
    big = 1 << 16

    def fn(rp=p, kq=p, tl=p, T=1, X=p, w=2, ob=2, out_size=big):
        tail = (w, ob, p, out_size, None) if which == "bit" else (w, p, out_size, None)
        return getattr(lib, "qgtc_tiledmm2" + which)(rp, kq, tl, T, 100, X, big, 8, *tail)

    assert fn(rp=None, kq=None, tl=None, T=0) == EINVAL       # no row_ptr, no tiles
    assert fn(rp=None, T=0) == EINVAL
    assert fn(w=9, out_size=10) == EINVAL                     # bit2 > 8 and a short output
    assert fn(X=p + 4, out_size=10) == EALIGN                 # X off a 16-byte boundary and a short output
    if which == "bit":
        assert fn(X=p + 4, ob=33) == EALIGN                   # the shared check (X misaligned) comes before the entry's own (output_bit)
