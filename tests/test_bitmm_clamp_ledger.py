"""The ledger of bit-GEMM kernels x output layouts x requantiser branches: which cells bitmm_clamp_cases.CLAMP_CASES compares with the
oracle on sums next to the clamp, and that the cases are what they claim to be. Host logic only (the route queries, NumPy, the C oracle):
no GPU. tests/test_bitmm_clamp_gpu.py runs the same table on the device.

    python -m pytest tests/test_bitmm_clamp_ledger.py -s -k ledger      # prints the table: route | mode | ob class | cases
"""
import itertools
import os

import numpy as np
import pytest

import bitmm_clamp_cases as B

ALL_ROUTES = B.SINGLE_ROUTES + B.GROUPED_ROUTES
ALL_CELLS = set(itertools.product(ALL_ROUTES, (0, 1), B.OB_CLASSES))
IDS = [B.case_id(c) for c in B.CLAMP_CASES]


@pytest.fixture(scope="module")
def lib():
    import qgtc_ppopp22_amd

    assert os.path.exists(qgtc_ppopp22_amd.lib_path()), "libqgtc_hip.so is not built (run __graft_entry__.build())"
    from qgtc_ppopp22_amd import cabi

    return cabi.load()


def route_of(lib, c):
    q = lib.qgtc_bitmm_route if c.form == "single" else lib.qgtc_bitmm_batched_route
    return q(c.M, c.K, c.N, c.a, c.w, c.ob, c.mode, B.route_flags(c)).decode()


def test_ledger_covers_every_reachable_cell(lib):
    """Every cell of {kernel} x {rows, cols layout} x {ob class} has a case whose route query names that kernel, or stands in UNREACHABLE
    with the rule that excludes it; no case lands in a cell listed as unreachable."""
    assert set(B.UNREACHABLE) <= ALL_CELLS and all(isinstance(r, str) and r for r in B.UNREACHABLE.values())
    cells = {}
    for c in B.CLAMP_CASES:
        assert c.form in B.FORMS and c.engine in B.ENGINE_FLAGS and c.mode in (0, 1)
        assert (c.route in B.SINGLE_ROUTES) == (c.form == "single") and c.route in ALL_ROUTES
        assert route_of(lib, c) == c.route, B.case_id(c)
        cells.setdefault((c.route, c.mode, B.ob_class(c.ob)), []).append(B.case_id(c))
    print()
    for cell in sorted(ALL_CELLS, key=lambda t: (ALL_ROUTES.index(t[0]), t[1], B.OB_CLASSES.index(t[2]))):
        what = ", ".join(cells[cell]) if cell in cells else "UNREACHABLE: " + B.UNREACHABLE.get(cell, "?")
        print(f"{cell[0]} | {cell[1]} | {cell[2]} | {what}")
    reached_but_listed = sorted(set(cells) & set(B.UNREACHABLE))
    assert not reached_but_listed, f"listed as unreachable, yet a case gets there: {reached_but_listed}"
    holes = sorted(ALL_CELLS - set(cells) - set(B.UNREACHABLE))
    assert not holes, f"no case and no reason: {holes}"


def test_unreachable_cells_are_not_reached_by_any_query(lib):
    """A sweep of both route queries over shapes, plane counts, widths, engines and flags: every name they return is in the ledger, and no
    answer falls into a cell the ledger lists as unreachable."""
    seen = set()
    shapes = [(37, 100, 35), (37, 128, 128), (1213, 128, 128), (37, 515, 35), (37, 515, 70), (37, 515, 261), (300, 1100, 64), (70, 4225, 33),
              (9000, 4225, 64), (20000, 9000, 16)]
    planes = [(1, 1), (1, 2), (2, 2), (2, 1), (1, 4), (4, 1), (3, 3), (4, 4), (2, 8), (8, 2), (5, 5), (8, 8), (9, 1), (1, 9), (32, 32)]
    for (M, K, N), (a, w), mode, ob in itertools.product(shapes, planes, (0, 1), (1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 23)):
        for eng, zs in itertools.product(B.ENGINE_FLAGS.values(), (0, B.NO_ZERO_SKIP)):
            name = lib.qgtc_bitmm_route(M, K, N, a, w, ob, mode, eng | zs).decode()
            assert name in B.SINGLE_ROUTES, name
            seen.add((name, mode, B.ob_class(ob)))
            name = lib.qgtc_bitmm_batched_route(M, K, N, a, w, ob, mode, eng | zs | B.ZERO_JUMP).decode()
            assert name in B.GROUPED_ROUTES, name
            seen.add((name, mode, B.ob_class(ob)))
            name = lib.qgtc_bitmm_batched_route(M, K, N, a, w, ob, mode, eng | zs).decode()
            assert name in B.GROUPED_ROUTES, name
            seen.add((name, mode, B.ob_class(ob)))
    assert not seen & set(B.UNREACHABLE), sorted(seen & set(B.UNREACHABLE))
    assert {s[0] for s in seen} == set(ALL_ROUTES)


def test_shapes_have_an_interior_and_a_ragged_tile():
    for c in B.CLAMP_CASES:
        assert c.M > 32 and c.M % 32 and c.N > 32 and c.N % 32 and c.K % 128, B.case_id(c)
        assert 1 <= c.ob <= 23 and (1 << c.ob) + 2 <= B.max_sum(c.K, c.a, c.w), B.case_id(c)
        if B.ob_class(c.ob) == "hi":
            assert c.ob == B.ob_hi(c.K, c.a, c.w), B.case_id(c)
    by = lambda r: [c for c in B.CLAMP_CASES if c.route == r]  # noqa: E731
    assert all(c.K > 4096 for c in by("k_bitmm_fp4_stream") + by("k_bitmm_fp4_skinny"))
    assert any(c.K == 4095 and c.ob == 11 for c in by("k_bitmm_fp4_one")) and any(c.ob >= 16 for c in by("k_bitmm_fp4_one"))
    assert all(c.a >= 9 and c.zero_skip for c in by("k_bitmm_planes"))
    assert any(c.K > 1024 for c in by("k_bitmm_planes"))                                           # more than one chunk of 8 k-quads
    assert any(c.a == 32 and 8 * 32 * ((c.K + 127) // 128) > 1024 for c in by("k_bitmm_planes"))   # the census loop's second trip
    # k_bitmm_fp4_wide's two bit epilogues, each forced by the plane counts: every ob class on both, in both layouts; the 4 x 2 one on both
    # sides of its `ob <= 4` test with the run-time widths, the 2 x 4 one on requant_pack16<1>, <2> and <0> below and above plane 8
    wide = by("k_bitmm_fp4_wide")
    for mode, cls in itertools.product((0, 1), B.OB_CLASSES):
        assert {B.wide_epilogue(c) for c in wide if c.mode == mode and B.ob_class(c.ob) == cls} >= {"4x2", "2x4"}, (mode, cls)
    assert {c.ob for c in wide if B.wide_epilogue(c) == "4x2"} >= {1, 2, 3, 4, 5, 6, 8} and {c.ob for c in wide if B.wide_epilogue(c) == "2x4"} >= {1, 2, 4, 7, 8}
    for r in ("k_bitmm_fp4_wide", "k_bitmm_fp4_rows_single", "k_bitmm_fp4_rows"):
        assert {B.ob_class(c.ob) for c in by(r) if c.ob <= 4} and {c.ob for c in by(r) if c.ob > 4}
    assert {c.form for c in B.CLAMP_CASES} == set(B.FORMS)


@pytest.mark.parametrize("c", B.CLAMP_CASES, ids=IDS)
def test_sums_sit_on_both_sides_of_the_clamp(c):
    """From the NumPy definition alone: every target sum is among the staircase's outputs, and outside the staircase at least a fifth of
    the sums lie strictly between 0 and 2^ob and at least a fifth strictly above it."""
    s = B.sums(c)
    rows, cols = B.staircase_rows(c), B.staircase_cols(c)
    stair = s[np.ix_(rows, cols)]
    lim = 1 << c.ob
    want = B.targets(c)
    assert set(want) >= {0, 1, lim - 1, lim, lim + 1, lim + 2, B.max_sum(c.K, c.a, c.w)}
    assert (2 * lim in want) == (2 * lim <= B.max_sum(c.K, c.a, c.w))
    for t in want:
        t32 = t & 0xFFFFFFFF
        t32 -= (1 << 32) if t32 >= (1 << 31) else 0          # (32-plane operands: the largest sum wraps the int32 accumulator)
        assert (stair == t32).any(), f"target sum {t} is missing"
    # ... and their stored values, which is what a comparison of outputs sees
    ref = B.reference(c)
    assert ref.min() >= 0 and ref.max() < lim
    assert {0, 1, lim - 1} <= set(ref[np.ix_(rows, cols)].reshape(-1).tolist())
    rest = np.ones(s.shape, dtype=bool)
    rest[rows, :] = False
    rest[:, cols] = False
    r = s[rest]
    below, above = ((r > 0) & (r < lim)).mean(), (r > lim).mean()
    assert below >= 0.2 and above >= 0.2, (below, above)
    assert lim / 2 <= np.median(r) <= 2 * lim, np.median(r)


@pytest.mark.parametrize("c", B.CLAMP_CASES, ids=IDS)
def test_oracle_agrees_with_the_numpy_rule(oracle, c):
    """The C oracle against the NumPy definition on exactly these inputs, in the layout of the case: a later mismatch on the device
    points at the kernel."""
    qx, qw = B.operands(c)
    assert qx.shape == (c.M, c.K) and qw.shape == (c.K, c.N)
    assert qx.min() >= 0 and qx.max() < (1 << c.a) and qw.min() >= 0 and qw.max() < (1 << c.w)
    X, Wt = oracle.pack(B.as_int32(qx), c.a, False), oracle.pack(B.as_int32(qw), c.w, True)
    words = oracle.bitmm2bit(X, Wt, c.M, c.K, c.N, c.a, c.w, c.ob, col=(c.mode == 1))
    got = oracle.bit2val(words, c.ob, c.M, c.N, c.mode == 1, False)
    np.testing.assert_array_equal(got.astype(np.int64), B.reference(c))
    np.testing.assert_array_equal(oracle.acc(X, Wt, c.M, c.K, c.N, c.a, c.w).astype(np.int64), B.sums(c))
