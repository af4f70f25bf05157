"""C-ABI of the fused walk and product (include/qgtc_fused.h: qgtc_tiledmm_u8_linear): the header parses with cabi.signatures(text) to its
golden listing, the entry is exported and bound by cabi.load() at ABI 11, and bad arguments are refused before any device work in the
stated order: invalid, then misaligned, then short. Every call carries a bad argument and a NULL stream: nothing is launched."""
import ctypes
import os

import pytest

from qgtc_ppopp22_amd import cabi
from test_cabi import _lines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESIZE, EALIGN = 1, 2, 3
n, K, N2, LDK = 300, 62, 10, 64         # PAD4(K) = 64, PAD4(N2) = 12, S128(n) * 4 = 12 mask words
QB, OB = (n - 1) * 64 + 64, (n - 1) * 12 + 12


def fused_signatures():
    with open(cabi.FUSED_HEADER) as f:
        return cabi.signatures(f.read())


@pytest.fixture(scope="module")
def lib():
    return cabi.load()


@pytest.fixture(scope="module")
def p():
    b = (ctypes.c_uint32 * (1 << 16))()
    yield (ctypes.addressof(b) + 255) & ~255   # 256-byte aligned address inside the buffer
    del b


def test_the_header_parses_to_its_golden_listing():
    sig = fused_signatures()
    golden = open(os.path.join(ROOT, "tests", "golden", "qgtc_fused_abi.txt")).read().splitlines()
    assert list(sig) == ["qgtc_tiledmm_u8_linear"] and _lines(sig) == golden
    assert sig["qgtc_tiledmm_u8_linear"][1][-1] is ctypes.c_void_p    # the stream comes last


def test_the_entry_is_exported_and_bound(lib):
    for name, (ret, args) in fused_signatures().items():
        fn = getattr(lib, name)
        assert fn.restype is ret and list(fn.argtypes) == args, name
    assert lib.qgtc_abi_version() == 11
    assert "#define QGTC_ABI_VERSION 11" in open(cabi.HEADER).read()


def call(lib, p, codes_out, view=0, tiles=0, T=5, n=n, Q=0, ld=64, qn=QB, K=K, tq=0, ars=0, hq=0, hb=8, ct=0, ldk=LDK, cn=N2 * LDK, N2=N2, qb=0,
         g=N2, cs=0, lrs=0, bias=0, out="d", on=n * N2, oq="d", ldo=12, obn=OB, oqp=0, ob=8, rm=0, sm=0, mw=12):
    """offsets into the buffer, None for NULL; "d": the output of the table's kind"""
    out, oq = ((None if codes_out else 0) if out == "d" else out), ((0 if codes_out else None) if oq == "d" else oq)
    ptr = lambda off: None if off is None else p + off   # noqa: E731
    return lib.qgtc_tiledmm_u8_linear(ptr(view), ptr(view), ptr(tiles), T, n, ptr(Q), ld, qn, K, ptr(tq), ptr(ars), ptr(hq), hb, ptr(ct), ldk, cn,
                                      N2, ptr(qb), g, ptr(cs), ptr(lrs), ptr(bias), 0, ptr(out), on, ptr(oq), ldo, obn, ptr(oqp), ob, ptr(rm),
                                      ptr(sm), mw, None)


COMMON = {
    EINVAL: [dict(Q=None), dict(tq=None), dict(hq=None), dict(ct=None), dict(qb=None), dict(cs=None), dict(K=0), dict(K=257, ld=260, ldk=272),
             dict(N2=0), dict(N2=257, g=257), dict(hb=0), dict(hb=9), dict(g=2), dict(n=0), dict(T=-1), dict(view=None), dict(tiles=None),
             dict(out=0, oq=0), dict(out=None, oq=None), dict(K=257, Q=1), dict(N2=0, cn=0), dict(hb=9, tq=4)],
    EALIGN: [dict(Q=1), dict(ld=62), dict(ld=60), dict(tq=4), dict(hq=8), dict(ars=2), dict(ct=4), dict(ldk=48), dict(ldk=72), dict(qb=8),
             dict(cs=2), dict(lrs=2), dict(bias=2), dict(rm=4), dict(sm=8), dict(tiles=4), dict(Q=1, qn=0), dict(tq=4, mw=0)],
    ESIZE: [dict(qn=QB - 1), dict(cn=N2 * LDK - 1), dict(ldk=128), dict(mw=11), dict(mw=11, rm=None), dict(Q=4, qn=QB - 4)],
}
FLOAT_OUT = {EINVAL: [], EALIGN: [dict(out=2)], ESIZE: [dict(on=n * N2 - 1), dict(on=0)]}
CODES_OUT = {EINVAL: [dict(oqp=None), dict(ob=0), dict(ob=9)], EALIGN: [dict(oq=2), dict(ldo=8), dict(ldo=10), dict(ldo=14), dict(oqp=4),
                                                                       dict(ldo=14, obn=0)],
             ESIZE: [dict(obn=OB - 1), dict(obn=0), dict(ldo=16)]}


@pytest.mark.parametrize("codes_out", [False, True], ids=["float", "codes"])
def test_bad_arguments_are_refused_in_the_stated_order(lib, p, codes_out):
    for table in (COMMON, CODES_OUT if codes_out else FLOAT_OUT):
        for want, cases in table.items():
            for kw in cases:
                assert call(lib, p, codes_out, **kw) == want, (codes_out, kw)
