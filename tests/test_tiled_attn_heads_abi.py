"""C-ABI of the multi-head entries of the attention path (include/qgtc_attn_heads.h: the product and the score gradient on both views,
plain, under the edge-dropout mask and under the node masks, and the row dot - thirteen entries, each its single-head twin of qgtc.h
with `int heads` after the twin's own arguments, before the mask's and the stream): the header parses with cabi.signatures(text), every
entry is exported and bound by cabi.load(), the header's own golden file holds, the first two headers and ABI version 11 are untouched,
and bad arguments are refused before any device work with the twin's code in the twin's order - invalid, then misaligned, then short -
plus the refusals of `heads` (no GPU needed)."""
import ctypes
import os

import pytest

from qgtc_ppopp22_amd import cabi
from test_cabi import _lines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, ESIZE, EALIGN = 0, 1, 2, 3
MASK_ARGS = {"": [], "_drop": [ctypes.c_uint32, ctypes.c_uint64], "_nodes": [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]}
# the entry with heads -> (the entry of qgtc.h it generalises, the mask's arguments)
TWINS = {}
for _mask in ("", "_drop", "_nodes"):
    for _stem in ("qgtc_tiledatt", "qgtc_tiledatt_grad"):
        for _t in ("", "_t"):
            TWINS[f"{_stem}_heads_f32{_t}{_mask}"] = (f"{_stem}_f32{_t}{_mask}", MASK_ARGS[_mask])
    if not _mask:
        TWINS["qgtc_rowdot_heads_f32"] = ("qgtc_rowdot_f32", [])


def attn_heads_signatures():
    with open(cabi.ATTN_HEADS_HEADER) as f:
        return cabi.signatures(f.read())


@pytest.fixture(scope="module")
def lib():
    return cabi.load()


@pytest.fixture(scope="module")
def p():
    b = (ctypes.c_uint32 * ((1 << 16) + 64))()
    addr = (ctypes.addressof(b) + 255) & ~255   # 256-byte aligned address inside the buffer
    yield addr
    del b


def test_the_header_parses_to_the_thirteen_entries_and_each_is_its_twin_plus_heads():
    sig, base = attn_heads_signatures(), cabi.signatures()
    assert len(TWINS) == 13 and set(sig) == set(TWINS) and len(sig) == 13
    for name, (twin, mask) in TWINS.items():
        ret, args = sig[name]
        tret, targs = base[twin]
        k = len(mask) + 1   # the mask's arguments and the stream
        assert targs[len(targs) - k:] == mask + [ctypes.c_void_p], twin
        assert ret is tret and args == targs[:len(targs) - k] + [ctypes.c_int] + mask + [ctypes.c_void_p], name


def test_the_golden_file_holds():
    golden = open(os.path.join(ROOT, "tests", "golden", "qgtc_attn_heads_abi.txt")).read().splitlines()
    assert _lines(attn_heads_signatures()) == golden


def test_every_entry_is_exported_and_bound(lib):
    for name, (ret, args) in attn_heads_signatures().items():
        fn = getattr(lib, name)
        assert fn.restype is ret and list(fn.argtypes) == args, name


def test_the_first_two_headers_are_untouched(lib):
    sig = cabi.signatures()
    with open(cabi.HEADS_HEADER) as f:
        heads_text = f.read()
    assert not set(sig) & set(TWINS) and not set(cabi.signatures(heads_text)) & set(TWINS)
    assert "qgtc_attn_heads" not in open(cabi.HEADER).read() and "qgtc_attn_heads" not in heads_text
    assert lib.qgtc_abi_version() == 11
    assert "#define QGTC_ABI_VERSION 11" in open(cabi.HEADER).read()
    golden = os.path.join(ROOT, "tests", "golden")
    assert _lines(sig) == open(os.path.join(golden, "qgtc_abi.txt")).read().splitlines()
    assert _lines(cabi.signatures(heads_text)) == open(os.path.join(golden, "qgtc_heads_abi.txt")).read().splitlines()


@pytest.mark.parametrize("mask", ["", "_drop", "_nodes"])
@pytest.mark.parametrize("grad", [False, True])
@pytest.mark.parametrize("transposed", [False, True])
def test_attention_entries_refuse_what_their_twins_refuse_in_their_order(lib, p, transposed, grad, mask):
    big = 1 << 16
    stem = "qgtc_tiledatt_grad" if grad else "qgtc_tiledatt"
    sfx = ("_t" if transposed else "") + mask
    heads_entry, twin = getattr(lib, f"{stem}_heads_f32{sfx}"), getattr(lib, f"{stem}_f32{sfx}")
    vectors = ("own", "nbr", "m", "inv", "D") if grad else ("own", "nbr", "shift", "m", "inv")
    ok = (p,) * (4 if transposed else 3)
    none = (None,) * len(ok)

    def call(entry, heads, idx=ok, T=1, n=100, N=8, x_elems=big, out_elems=big, X=p, out=p, other=p, slope=0.2, flag=0, tail=None, **vec):
        v = {name: vec.pop(name, p) for name in vectors}
        assert not vec, vec
        if tail is None:
            tail = {"": (), "_drop": (1 << 31, 7), "_nodes": (p, p, 4)}[mask]
        h = () if heads is None else (heads,)
        if grad:
            return entry(*idx, T, n, X, other, x_elems, N, v["own"], v["nbr"], slope, flag, v["m"], v["inv"], v["D"], out, out_elems, *h,
                         *tail, None)
        return entry(*idx, T, n, X, x_elems, N, v["own"], v["nbr"], slope, flag, v["shift"], v["m"], v["inv"], out, out_elems, *h, *tail, None)

    cases = [dict(n=0), dict(n=-5), dict(n=(1 << 23) + 1), dict(N=0), dict(N=-4), dict(T=-1), dict(X=None), dict(out=None),
             dict(idx=none, T=0, X=None), dict(idx=none, T=0, out=None), dict(x_elems=799), dict(out_elems=99),
             dict(n=1 << 23, N=1 << 20, x_elems=(1 << 43) - 1, out_elems=1 << 43), dict(idx=ok[:-1] + (p + 4,)),
             dict(idx=ok[:-1] + (p + 4,), out_elems=99), dict(X=p + 1), dict(out=p + 2), dict(slope=-0.001), dict(slope=float("nan")),
             dict(idx=none, T=0, slope=2.0), dict(flag=-1), dict(flag=2), dict(X=p + 1, slope=2.0, x_elems=1), dict(X=p + 1, x_elems=1),
             dict(other=None), dict(other=p + 2), dict(x_elems=799, flag=1)]
    cases += [dict(idx=ok[:k] + (None,) + ok[k + 1:]) for k in range(len(ok))]
    for flag in (0, 1):
        for name in vectors:
            if not grad and name == "m" and flag == 1:
                continue                                      # the backward mode does not touch m
            cases += [dict(flag=flag, **{name: None}), dict(idx=none, T=0, flag=flag, **{name: None}), dict(flag=flag, **{name: p + 2}),
                      dict(flag=flag, x_elems=799, **{name: p + 2})]
    if mask == "_nodes":
        cases += [dict(tail=(p, p, 3)), dict(tail=(None, p, 3)), dict(tail=(p + 4, p, 4)), dict(tail=(p, p + 8, 4)), dict(tail=(p + 4, p, 3)),
                  dict(tail=(p, p, 3), X=p + 1), dict(tail=(p, p, 3), x_elems=799), dict(tail=(p + 4, p, 4), X=None)]
    seen = set()
    for kw in cases:
        if not grad and "other" in kw:
            continue
        want = call(twin, None, **kw)
        assert want != OK, kw
        seen.add(want)
        for heads in (1, 2):
            assert call(heads_entry, heads, **kw) == want, (kw, heads)
    assert seen == {EINVAL, ESIZE, EALIGN}
    # ---- what heads add: invalid, so before misaligned and short ----
    for heads in (0, -1, 3, 16):
        assert call(heads_entry, heads) == EINVAL, heads
        assert call(heads_entry, heads, X=p + 1) == EINVAL and call(heads_entry, heads, x_elems=799) == EINVAL
    assert call(heads_entry, 3, N=9, x_elems=899) == ESIZE      # 3 divides 9: the next refusal is reached
    assert call(heads_entry, 0, N=0) == EINVAL
    if grad:
        # the [n, H] output is checked in elements, n * heads
        assert call(heads_entry, 2, out_elems=199) == ESIZE and call(heads_entry, 8, out_elems=799) == ESIZE
        assert call(heads_entry, 1, out_elems=99) == ESIZE
        assert call(heads_entry, 65536, n=1, N=65536, x_elems=1 << 20) == EINVAL   # the heads ride a grid dimension
    else:
        assert call(heads_entry, 2, out_elems=799) == ESIZE


def test_rowdot_refuses_bad_arguments(lib, p):
    big = 1 << 16

    def fn(n=100, N=8, A=p, B=p, out=p, ab_elems=big, out_elems=big, heads=2):
        if heads is None:
            return lib.qgtc_rowdot_f32(A, B, ab_elems, n, N, out, out_elems, None)
        return lib.qgtc_rowdot_heads_f32(A, B, ab_elems, n, N, out, out_elems, heads, None)

    cases = [dict(n=0), dict(n=-1), dict(n=(1 << 23) + 1), dict(N=0), dict(N=-2), dict(ab_elems=799), dict(out_elems=99),
             dict(n=1 << 23, N=1 << 20, ab_elems=(1 << 43) - 1, out_elems=1 << 43), dict(A=p + 1, ab_elems=799), dict(A=None, B=p + 1)]
    for name in ("A", "B", "out"):
        cases += [{name: None}, {name: p + 1}, {name: p + 2}]
    for kw in cases:
        want = fn(heads=None, **kw)
        assert want != OK and fn(heads=1, **kw) == want and fn(heads=2, **kw) == want, kw
    for heads in (0, -1, 3, 16):
        assert fn(heads=heads) == EINVAL and fn(heads=heads, A=p + 1) == EINVAL and fn(heads=heads, ab_elems=799) == EINVAL
    assert fn(heads=2, out_elems=199) == ESIZE and fn(heads=8, out_elems=799) == ESIZE
