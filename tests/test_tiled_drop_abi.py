"""C-ABI of edge dropout (include/qgtc.h, "Edge dropout": qgtc_edge_kept and the eight _drop entries): the nine symbols are exported,
the ABI version stays 11, and every _drop entry refuses what its parent refuses, in the parent's order, before any device work (no GPU
needed). The signatures come from the header (cabi.load())."""
import ctypes
import os

import pytest

OK, EINVAL, ESIZE, EALIGN = 0, 1, 2, 3
NAMES = ("qgtc_edge_kept", "qgtc_tiledmm_f32_drop", "qgtc_tiledmm_f32_t_drop", "qgtc_tiledmax_f32_drop", "qgtc_tiledmax_f32_t_drop",
         "qgtc_tiledatt_f32_drop", "qgtc_tiledatt_f32_t_drop", "qgtc_tiledatt_grad_f32_drop", "qgtc_tiledatt_grad_f32_t_drop")
MASK = (1 << 31, 0x0123456789ABCDEF)   # threshold, seed: any value of either is valid


@pytest.fixture(scope="module")
def lib():
    from qgtc_ppopp22_amd import cabi

    return cabi.load()


def _buf(words):
    b = (ctypes.c_uint32 * (words + 64))()
    addr = ctypes.addressof(b)
    return b, (addr + 255) & ~255   # keep the buffer alive; 256-byte aligned address inside it


def test_symbols_and_version(lib):
    for name in NAMES:
        assert getattr(lib, name), name
    assert len(NAMES) == 9
    assert lib.qgtc_abi_version() == 11


def test_the_header_declares_the_entries():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qgtc.h")).read()
    assert "Edge dropout" in text
    for name in NAMES:
        assert f"int {name}(" in text, name
    assert "#define QGTC_ABI_VERSION 11" in text
    for name in NAMES[1:]:   # `threshold, seed` sit before `stream`
        decl = text[text.index(f"int {name}("):]
        decl = " ".join(decl[: decl.index(";")].split())
        assert decl.endswith("uint32_t threshold, uint64_t seed, void *stream)"), name


def test_edge_kept_needs_no_device_and_takes_full_width_arguments(lib):
    # threshold 0 keeps everything; the largest threshold keeps only H = 2^32 - 1
    for i, j, seed in ((0, 0, 0), (2 ** 32 - 1, 2 ** 32 - 1, 2 ** 64 - 1), (5, 7, 1)):
        assert lib.qgtc_edge_kept(i, j, seed, 0) == 1
    # H(0, 0, 0) = 0x01fce552 (the header's rule; tests/test_tiled_drop_model.py has the known answers)
    assert lib.qgtc_edge_kept(0, 0, 0, 0x01FCE552) == 1
    assert lib.qgtc_edge_kept(0, 0, 0, 0x01FCE553) == 0
    assert lib.qgtc_edge_kept(0, 0, 1, 0xA263E079) == 1 and lib.qgtc_edge_kept(0, 0, 1, 0xA263E07A) == 0
    # both seed words arrive: H(0, 0, 0x0123456789ABCDEF) = 0x403f6c8a, H(0, 0, 2^64 - 1) = 0xd39d7ce6
    assert lib.qgtc_edge_kept(0, 0, 0x0123456789ABCDEF, 0x403F6C8A) == 1 and lib.qgtc_edge_kept(0, 0, 0x0123456789ABCDEF, 0x403F6C8B) == 0
    assert lib.qgtc_edge_kept(0, 0, 2 ** 64 - 1, 0xD39D7CE6) == 1 and lib.qgtc_edge_kept(0, 0, 2 ** 64 - 1, 0xD39D7CE7) == 0


def _common_refusals(fn, ok, none, out_short):
    """the refusals every float entry shares (tiled_f32_args_ok), through fn(idx, T, n, N, **kw)"""
    p = ok[0]
    assert fn(ok, 1, 0, 8) == EINVAL                          # n < 1
    assert fn(ok, 1, -5, 8) == EINVAL
    assert fn(ok, 1, (1 << 23) + 1, 8) == EINVAL              # n > 2^23
    assert fn(ok, 1, 100, 0) == EINVAL                        # N < 1
    assert fn(ok, 1, 100, -3) == EINVAL
    assert fn(ok, -1, 100, 8) == EINVAL                       # negative n_tiles
    for k in range(len(ok)):                                  # tiles without one of the index arrays or the tile words
        assert fn(ok[:k] + (None,) + ok[k + 1:], 1, 100, 8) == EINVAL, k
    assert fn(ok, 1, 100, 8, X=None) == EINVAL                # no X / A
    assert fn(ok, 1, 100, 8, out=None) == EINVAL              # no out
    assert fn(none, 0, 100, 8, X=None) == EINVAL              # ... also without tiles
    assert fn(none, 0, 100, 8, out=None) == EINVAL
    assert fn(ok, 1, 100, 8, x_elems=799) == ESIZE            # one float short of 100 x 8
    assert fn(ok, 1, 100, 8, out_elems=out_short) == ESIZE
    assert fn(ok, 1, 1 << 23, 1 << 20, x_elems=(1 << 43) - 1, out_elems=1 << 43) == ESIZE     # n * N does not wrap
    assert fn(ok[:-1] + (p + 4,), 1, 100, 8) == EALIGN        # tiles off a 16-byte boundary
    assert fn(ok[:-1] + (p + 8,), 1, 100, 8) == EALIGN
    for off in (1, 2, 3):
        assert fn(ok, 1, 100, 8, X=p + off) == EALIGN         # X / A off a 4-byte boundary
        assert fn(ok, 1, 100, 8, out=p + off) == EALIGN       # out off a 4-byte boundary
    assert fn(ok, 1, 100, 8, X=p + 1, x_elems=1) == EALIGN    # misaligned beats short
    assert fn(ok, 1, 0, 8, X=p + 1, x_elems=1) == EINVAL      # invalid beats both


@pytest.mark.parametrize("transposed", [False, True])
def test_float_drop_entries_refuse_bad_arguments(lib, transposed):
    keep, p = _buf(1 << 16)
    big = 1 << 16
    entry = lib.qgtc_tiledmm_f32_t_drop if transposed else lib.qgtc_tiledmm_f32_drop

    def fn(idx, T, n, N, x_elems=big, out_elems=big, X=p, out=p, row_scale=None, src_scale=None, mask=MASK):
        return entry(*idx, T, n, X, x_elems, N, row_scale, src_scale, out, out_elems, *mask, None)

    ok = (p,) * (4 if transposed else 3)
    none = (None,) * len(ok)
    _common_refusals(fn, ok, none, 799)
    for name in ("row_scale", "src_scale"):                   # both scales are optional, and aligned when given
        for off in (1, 2, 3):
            assert fn(ok, 1, 100, 8, **{name: p + off}) == EALIGN, name
            assert fn(none, 0, 100, 8, **{name: p + off}) == EALIGN, name
        assert fn(ok, 1, 100, 8, x_elems=799, **{name: p}) == ESIZE
        assert fn(ok, 1, 0, 8, **{name: p + 1}) == EINVAL
    for mask in ((0, 0), (2 ** 32 - 1, 2 ** 64 - 1)):         # no threshold or seed is refused, and none lifts a refusal
        assert fn(ok, 1, 0, 8, mask=mask) == EINVAL
        assert fn(ok, 1, 100, 8, x_elems=799, mask=mask) == ESIZE


@pytest.mark.parametrize("transposed", [False, True])
def test_max_drop_entries_refuse_bad_arguments(lib, transposed):
    keep, p = _buf(1 << 16)
    big = 1 << 16
    entry = lib.qgtc_tiledmax_f32_t_drop if transposed else lib.qgtc_tiledmax_f32_drop

    def fn(idx, T, n, N, x_elems=big, out_elems=big, X=p, out=p, op=0, arg=None, arg_elems=0, mask=MASK):
        return entry(*idx, T, n, X, x_elems, N, op, out, out_elems, arg, arg_elems, *mask, None)

    ok = (p,) * (4 if transposed else 3)
    none = (None,) * len(ok)
    _common_refusals(fn, ok, none, 799)
    for op in (-1, 2, 9):
        assert fn(ok, 1, 100, 8, op=op) == EINVAL             # op outside {0, 1}
        assert fn(none, 0, 100, 8, op=op) == EINVAL
    for op in (0, 1):
        for off in (1, 2, 3):
            assert fn(ok, 1, 100, 8, op=op, arg=p + off, arg_elems=big) == EALIGN
        assert fn(ok, 1, 100, 8, op=op, arg=p, arg_elems=799) == ESIZE
        assert fn(ok, 1, 100, 8, op=op, arg=p + 1, arg_elems=799) == EALIGN      # misaligned beats short
        assert fn(ok, 1, 100, 8, op=op, arg=p + 1, out=None) == EINVAL           # invalid beats misaligned
    assert fn(ok, 1, 100, 8, op=3, X=p + 1, x_elems=1) == EINVAL


@pytest.mark.parametrize("grad", [False, True])
@pytest.mark.parametrize("transposed", [False, True])
def test_attention_drop_entries_refuse_bad_arguments(lib, transposed, grad):
    keep, p = _buf(1 << 16)
    big = 1 << 16
    entry = getattr(lib, ("qgtc_tiledatt_grad_f32" if grad else "qgtc_tiledatt_f32") + ("_t" if transposed else "") + "_drop")
    vectors = ("own", "nbr", "m", "inv", "D") if grad else ("own", "nbr", "shift", "m", "inv")

    def fn(idx, T, n, N, x_elems=big, out_elems=big, X=p, out=p, other=p, slope=0.2, flag=0, mask=MASK, **vec):
        v = {name: vec.pop(name, p) for name in vectors}
        assert not vec, vec
        if grad:
            return entry(*idx, T, n, X, other, x_elems, N, v["own"], v["nbr"], slope, flag, v["m"], v["inv"], v["D"], out, out_elems,
                         *mask, None)
        return entry(*idx, T, n, X, x_elems, N, v["own"], v["nbr"], slope, flag, v["shift"], v["m"], v["inv"], out, out_elems, *mask, None)

    ok = (p,) * (4 if transposed else 3)
    none = (None,) * len(ok)
    _common_refusals(fn, ok, none, 99 if grad else 799)
    for slope in (-0.001, 1.001, 2.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert fn(ok, 1, 100, 8, slope=slope) == EINVAL       # a slope outside [0, 1]
        assert fn(none, 0, 100, 8, slope=slope) == EINVAL
    for flag in (-1, 2, 7):
        assert fn(ok, 1, 100, 8, flag=flag) == EINVAL         # backward / nbr_owns outside {0, 1}
    for flag in (0, 1):
        for name in vectors:
            if not grad and name == "m" and flag == 1:
                continue                                      # the backward mode does not touch m
            assert fn(ok, 1, 100, 8, flag=flag, **{name: None}) == EINVAL, (name, flag)
            assert fn(none, 0, 100, 8, flag=flag, **{name: None}) == EINVAL, (name, flag)
            for off in (1, 2, 3):
                assert fn(ok, 1, 100, 8, flag=flag, **{name: p + off}) == EALIGN, (name, flag)
        assert fn(ok, 1, 100, 8, flag=flag, x_elems=799) == ESIZE
    if grad:
        assert fn(ok, 1, 100, 8, other=None) == EINVAL        # the neighbours' matrix
        for off in (1, 2, 3):
            assert fn(ok, 1, 100, 8, other=p + off) == EALIGN
        assert fn(ok, 1, 100, 8, out_elems=100, x_elems=799) == ESIZE
    assert fn(ok, 1, 100, 8, X=p + 1, slope=2.0, x_elems=1) == EINVAL
    assert fn(ok, 1, 100, 8, X=p + 1, x_elems=1) == EALIGN
