"""C-ABI of the static affine chain (include/qgtc_chain.h: qgtc_affine_linear_chain, qgtc_tiledmm_u8_requant, qgtc_tiledmm_u8_t_requant):
the header parses with cabi.signatures(text) to its golden listing, every entry is exported and bound by cabi.load() at ABI 11, and bad
arguments are refused before any device work in the stated order: invalid (float in with float out included), then misaligned (a code
matrix off the 4-byte rule on either side), then short. Every call carries a bad argument and a NULL stream: nothing is launched."""
import ctypes
import os

import pytest

from qgtc_ppopp22_amd import cabi
from test_cabi import _lines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("qgtc_affine_linear_chain", "qgtc_tiledmm_u8_requant", "qgtc_tiledmm_u8_t_requant")
EINVAL, ESIZE, EALIGN = 1, 2, 3
M, K, N, LDK = 100, 62, 10, 64          # PAD4(K) = 64, PAD4(N) = 12
XB, OB = (M - 1) * 64 + 64, (M - 1) * 12 + 12
n, NW = 300, 62                         # the walks: PAD4(NW) = 64, S128(n) * 4 = 12 mask words
QB = (n - 1) * 64 + 64


def chain_signatures():
    with open(cabi.CHAIN_HEADER) as f:
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
    sig = chain_signatures()
    golden = open(os.path.join(ROOT, "tests", "golden", "qgtc_chain_abi.txt")).read().splitlines()
    assert list(sig) == list(ENTRIES) and _lines(sig) == golden
    assert all(args[-1] is ctypes.c_void_p for _, args in sig.values())    # the stream comes last


def test_every_entry_is_exported_and_bound(lib):
    for name, (ret, args) in chain_signatures().items():
        fn = getattr(lib, name)
        assert fn.restype is ret and list(fn.argtypes) == args, name
    assert lib.qgtc_abi_version() == 11
    assert "#define QGTC_ABI_VERSION 11" in open(cabi.HEADER).read()


def _product(kind):
    """the chain product with the left operand and the output of ``kind``: offsets into the buffer, None for NULL"""
    x0, xq0 = (0, None) if kind[0] == "f" else (None, 0)
    out0, oq0 = (0, None) if kind[1] == "f" else (None, 0)

    def call(lib, p, x=x0, xq=xq0, ldx=64, xn=XB, M=M, K=K, qa=0, ab=8, ct=0, ldk=LDK, cn=N * LDK, N=N, qb=0, g=N, cs=0, rs=0, bias=0,
             out=out0, on=M * N, oq=oq0, ldo=12, obn=OB, oqp=0, ob=8):
        ptr = lambda off: None if off is None else p + off
        return lib.qgtc_affine_linear_chain(ptr(x), ptr(xq), ldx, xn, M, K, ptr(qa), ab, ptr(ct), ldk, cn, N, ptr(qb), g, ptr(cs), ptr(rs),
                                            ptr(bias), 0, ptr(out), on, ptr(oq), ldo, obn, ptr(oqp), ob, None)
    return call


def _walk(transposed):
    def call(lib, p, view=0, T=5, n=n, Q=0, ld=64, qn=QB, N=NW, qp=0, rs=0, oqp=0, ob=8, oq=0, ldo=64, obn=QB, rm=0, sm=0, mw=12, tiles=0):
        ptr = lambda off: None if off is None else p + off
        fn = getattr(lib, "qgtc_tiledmm_u8" + ("_t" if transposed else "") + "_requant")
        return fn(*[ptr(view)] * (3 if transposed else 2), ptr(tiles), T, n, ptr(Q), ld, qn, N, ptr(qp), ptr(rs), ptr(oqp),
                  ob, ptr(oq), ldo, obn, ptr(rm), ptr(sm), mw, None)
    return call


COMMON = {   # every product, whatever its operands
    EINVAL: [dict(qa=None), dict(ct=None), dict(qb=None), dict(cs=None), dict(M=0), dict(K=0), dict(N=0), dict(ab=0), dict(ab=9), dict(g=2),
             dict(K=131072, ldk=131072, ldx=131072), dict(g=2, qa=4), dict(M=0, cn=0)],
    EALIGN: [dict(qa=4), dict(qb=8), dict(ct=4), dict(ldk=48), dict(ldk=72), dict(cs=2), dict(rs=2), dict(bias=2), dict(qa=4, cn=0)],
    ESIZE: [dict(cn=N * LDK - 1), dict(ldk=128)],
}
CODES_IN = {EINVAL: [dict(x=0)], EALIGN: [dict(xq=1), dict(xq=2), dict(ldx=60), dict(ldx=62), dict(ldx=66), dict(ldx=62, xn=0)],
            ESIZE: [dict(xn=XB - 1), dict(xn=0), dict(ldx=128), dict(xq=4, xn=XB - 4)]}
CODES_OUT = {EINVAL: [dict(out=0), dict(oqp=None), dict(ob=0), dict(ob=9), dict(oq=None)],
             EALIGN: [dict(oq=2), dict(ldo=8), dict(ldo=10), dict(ldo=14), dict(oqp=4), dict(ldo=14, obn=0)],
             ESIZE: [dict(obn=OB - 1), dict(obn=0), dict(ldo=16)]}
FLOAT_IN = {EINVAL: [dict(xq=0), dict(x=None)], EALIGN: [dict(x=2)], ESIZE: []}
FLOAT_OUT = {EINVAL: [dict(oq=0), dict(out=None)], EALIGN: [dict(out=2)], ESIZE: [dict(on=M * N - 1), dict(on=0)]}
WALK = {
    EINVAL: [dict(Q=None), dict(oq=None), dict(qp=None), dict(oqp=None), dict(N=0), dict(N=-1), dict(n=0), dict(T=-1), dict(ob=0), dict(ob=9),
             dict(view=None), dict(tiles=None), dict(N=0, Q=1), dict(ob=9, ldo=62), dict(n=0, obn=0)],
    EALIGN: [dict(Q=1), dict(ld=62), dict(oq=2), dict(ldo=60), dict(ldo=62), dict(ldo=66), dict(qp=4), dict(oqp=8), dict(rs=2), dict(rm=4),
             dict(sm=8), dict(tiles=4), dict(ldo=62, obn=0), dict(oq=2, mw=0)],
    ESIZE: [dict(qn=QB - 1), dict(obn=QB - 1), dict(obn=0), dict(ldo=128), dict(mw=11), dict(mw=11, rm=None), dict(oq=4, obn=QB - 4),
            dict(view=None, tiles=None, T=0, obn=0)],
}
TABLES = {"float-codes": (_product("fq"), COMMON, FLOAT_IN, CODES_OUT), "codes-codes": (_product("qq"), COMMON, CODES_IN, CODES_OUT),
          "codes-float": (_product("qf"), COMMON, CODES_IN, FLOAT_OUT), "float-float": (_product("ff"), {EINVAL: [dict(), dict(qa=4), dict(on=0)]}),
          "walk": (_walk(False), WALK), "walk-t": (_walk(True), WALK)}


@pytest.mark.parametrize("which", TABLES)
def test_bad_arguments_are_refused_in_the_stated_order(lib, p, which):
    call, *tables = TABLES[which]
    for table in tables:
        for want, cases in table.items():
            for kw in cases:
                assert call(lib, p, **kw) == want, (which, kw)
