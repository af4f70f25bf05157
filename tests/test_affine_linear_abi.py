"""C-ABI of the byte-code linear route (include/qgtc_linear.h: qgtc_affine_pack_weight, qgtc_affine_linear_u8): the header parses with
cabi.signatures(text) to the two entries and equals its own golden file, both are exported and bound by cabi.load(), and bad arguments
are refused before any device work in the stated order: invalid (K above QGTC_LINEAR_K_MAX included), then misaligned, then short.
Every call here carries a bad argument and a NULL stream: nothing is launched (no GPU needed)."""
import ctypes
import os

import pytest

from qgtc_ppopp22_amd import cabi
from test_cabi import _lines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("qgtc_affine_pack_weight", "qgtc_affine_linear_u8")
EINVAL, ESIZE, EALIGN = 1, 2, 3
K_MAX = 131071
M, K, N, LDK = 100, 62, 10, 64


def linear_signatures():
    with open(cabi.LINEAR_HEADER) as f:
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
    sig = linear_signatures()
    golden = open(os.path.join(ROOT, "tests", "golden", "qgtc_linear_abi.txt")).read().splitlines()
    assert list(sig) == list(ENTRIES) and _lines(sig) == golden
    assert all(args[-1] is ctypes.c_void_p for _, args in sig.values())    # the stream comes last
    assert f"#define QGTC_LINEAR_K_MAX {K_MAX}\n" in open(cabi.LINEAR_HEADER).read()


def test_every_entry_is_exported_and_bound(lib):
    for name, (ret, args) in linear_signatures().items():
        fn = getattr(lib, name)
        assert fn.restype is ret and list(fn.argtypes) == args, name
    assert lib.qgtc_abi_version() == 11


def _pack(lib, p, w=0, K=K, N=N, b=4, pc=1, qp=0, qn=4 * N, ct=0, ldk=LDK, cn=N * LDK, cs=0, sn=N):
    ptr = lambda off: None if off is None else p + off
    return lib.qgtc_affine_pack_weight(ptr(w), K, N, b, pc, ptr(qp), qn, ptr(ct), ldk, cn, ptr(cs), sn, None)


def _linear(lib, p, x=0, M=M, K=K, qa=0, ab=8, ct=0, ldk=LDK, cn=N * LDK, N=N, qb=0, g=N, cs=0, rs=0, bias=0, out=0, on=M * N):
    ptr = lambda off: None if off is None else p + off
    return lib.qgtc_affine_linear_u8(ptr(x), M, K, ptr(qa), ab, ptr(ct), ldk, cn, N, ptr(qb), g, ptr(cs), ptr(rs), ptr(bias), 0, ptr(out), on, None)


REFUSALS = {
    "qgtc_affine_pack_weight": (_pack, {
        EINVAL: [dict(w=None), dict(qp=None), dict(ct=None), dict(cs=None), dict(K=0), dict(N=0), dict(N=-1), dict(b=0), dict(b=9),
                 dict(K=K_MAX + 1, ldk=K_MAX + 1), dict(b=9, qp=4), dict(K=0, cn=0)],                    # invalid before the rest
        EALIGN: [dict(qp=4), dict(qp=8), dict(ct=4), dict(ct=8), dict(ldk=48), dict(ldk=72), dict(ldk=63), dict(w=2), dict(cs=2),
                 dict(ct=4, cn=0), dict(ldk=72, sn=0)],                                                  # misaligned before short
        ESIZE: [dict(qn=4 * N - 1), dict(pc=0, qn=3), dict(cn=N * LDK - 1), dict(sn=N - 1), dict(ldk=128), dict(ct=16, cn=0)],
    }),
    "qgtc_affine_linear_u8": (_linear, {
        EINVAL: [dict(x=None), dict(qa=None), dict(ct=None), dict(qb=None), dict(cs=None), dict(out=None), dict(M=0), dict(K=0), dict(N=0),
                 dict(ab=0), dict(ab=9), dict(g=0), dict(g=2), dict(g=N + 1), dict(K=K_MAX + 1, ldk=K_MAX + 1), dict(g=2, qa=4), dict(M=0, on=0)],
        EALIGN: [dict(qa=4), dict(qb=8), dict(ct=4), dict(ldk=48), dict(ldk=72), dict(x=2), dict(cs=2), dict(rs=2), dict(bias=2), dict(out=2),
                 dict(qa=4, on=0), dict(ldk=72, cn=0)],
        ESIZE: [dict(cn=N * LDK - 1), dict(on=M * N - 1), dict(on=0), dict(ldk=128), dict(x=4, on=0), dict(rs=None, bias=None, on=0)],
    }),
}


@pytest.mark.parametrize("entry", ENTRIES)
def test_bad_arguments_are_refused_in_the_stated_order(lib, p, entry):
    call, table = REFUSALS[entry]
    for want, cases in table.items():
        for kw in cases:
            assert call(lib, p, **kw) == want, (entry, kw)
