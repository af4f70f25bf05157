"""C-ABI of the edge-weighted sum on byte codes (include/qgtc_codes_edge.h): the header parses with cabi.signatures(text) to its golden
listing, the entries are exported and bound by cabi.load() at ABI 11, and bad arguments are refused before any device work in the stated
order: invalid, then misaligned, then short. Every call carries a bad argument and a NULL stream: nothing is launched."""
import ctypes
import os

import pytest

from qgtc_ppopp22_amd import cabi
from test_cabi import _lines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESIZE, EALIGN = 1, 2, 3
n, N = 300, 24                          # PAD4(N) = 24, S128(n) * 4 = 12 mask words
QB = (n - 1) * 24 + 24
NAMES = ["qgtc_tiledmm_u8_edge", "qgtc_tiledmm_u8_t_edge"]


def edge_signatures():
    with open(cabi.CODES_EDGE_HEADER) as f:
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
    sig = edge_signatures()
    golden = open(os.path.join(ROOT, "tests", "golden", "qgtc_codes_edge_abi.txt")).read().splitlines()
    assert list(sig) == NAMES and _lines(sig) == golden
    assert all(args[-1] is ctypes.c_void_p for _, args in sig.values())    # the stream comes last


def test_the_entries_are_exported_and_bound(lib):
    for name, (ret, args) in edge_signatures().items():
        fn = getattr(lib, name)
        assert fn.restype is ret and list(fn.argtypes) == args, name
    assert lib.qgtc_abi_version() == 11


def call(lib, p, kind, t, view=0, tiles=0, T=5, n=n, Q=0, ld=24, qn=QB, N=N, qp=0, rs=0, vp=0, vr=0, val=0, nv=100, heads=2, out="d",
         on=n * N, oq="d", ldo=24, obn=QB, oqp=0, ob=8, rm=0, sm=0, mw=12):
    """offsets into the buffer, None for NULL; "d": the destination of the kind ("float" or "codes")"""
    out, oq = ((0 if kind == "float" else None) if out == "d" else out), ((None if kind == "float" else 0) if oq == "d" else oq)
    ptr = lambda off: None if off is None else p + off   # noqa: E731
    head = (ptr(view),) * (3 if t else 2) + (ptr(tiles), T, n, ptr(Q), ld, qn, N)
    return getattr(lib, NAMES[t])(*head, ptr(qp), ptr(rs), ptr(vp), ptr(vr), ptr(val), nv, heads, ptr(out), on, ptr(oq), ldo, obn, ptr(oqp),
                                  ob, ptr(rm), ptr(sm), mw, None)


COMMON = {
    EINVAL: [dict(Q=None), dict(N=0), dict(n=0), dict(T=-1), dict(view=None), dict(tiles=None), dict(qp=None), dict(heads=0), dict(heads=5),
             dict(heads=4), dict(N=10, heads=2), dict(val=None), dict(vp=None), dict(vr=None), dict(nv=1 << 31), dict(heads=4, ld=14),
             dict(vp=None, val=2), dict(nv=1 << 31, qn=0), dict(val=None, vr=1)],
    EALIGN: [dict(Q=1), dict(ld=20), dict(ld=26), dict(rm=4), dict(sm=8), dict(tiles=4), dict(qp=4), dict(rs=2), dict(val=2), dict(vp=4),
             dict(vr=1), dict(val=2, qn=0), dict(vp=4, mw=0), dict(vr=1, qn=0)],
    ESIZE: [dict(qn=QB - 1), dict(mw=11), dict(mw=11, rm=None), dict(Q=4, qn=QB - 4)],
}
OWN = {
    "float": {EINVAL: [dict(out=None), dict(oq=0)], EALIGN: [dict(out=2)], ESIZE: [dict(on=n * N - 1)]},
    "codes": {EINVAL: [dict(oq=None), dict(out=0), dict(oqp=None), dict(ob=0), dict(ob=9)],
              EALIGN: [dict(oq=2), dict(ldo=26), dict(oqp=4), dict(ldo=26, obn=0)], ESIZE: [dict(obn=QB - 1), dict(ldo=28)]},
}


@pytest.mark.parametrize("t", [0, 1], ids=["adj", "adj.T"])
@pytest.mark.parametrize("kind", ["float", "codes"])
def test_bad_arguments_are_refused_in_the_stated_order(lib, p, kind, t):
    assert call(lib, p, kind, t, T=0, view=None, tiles=None, vp=None, vr=None, val=None, nv=0, qn=QB - 1) == ESIZE   # no tiles: NULLs pass
    for table in (COMMON, OWN[kind]):
        for want, cases in table.items():
            for kw in cases:
                assert call(lib, p, kind, t, **kw) == want, (kind, t, kw)
