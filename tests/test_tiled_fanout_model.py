"""The rule of fixed-fanout sampling (include/qgtc_fanout.h) on its NumPy model tests/tiled_fanout_model.py: the facts that make it
exact - distinct hashes within a row and within a column - and its stated consequences. No GPU."""
import numpy as np
import pytest

import tiled_drop_model as dm
import tiled_fanout_model as fm
from tiled_float_model import neighbour_lists
from tiled_model import random_edges, set_cells

GOLDEN64 = 0x9E3779B97F4A7C15


@pytest.mark.parametrize("seed", [0, 1])
def test_the_hashes_of_one_row_and_of_one_column_are_distinct(seed):
    """mix32 is a bijection, so j -> H(i, j, seed) and i -> H(i, j, seed) are: no duplicate over 2^17 ids, for i, j = 0 .. 7."""
    ids = np.arange(1 << 17, dtype=np.int64)
    for fixed in range(8):
        assert np.unique(dm.H(fixed, ids, seed)).size == ids.size, ("row", fixed)
        assert np.unique(dm.H(ids, fixed, seed)).size == ids.size, ("column", fixed)


def _graph(n, seed=0):
    rng = np.random.default_rng(100 + n + seed)
    return random_edges(rng, n, 6 * n + 5)


@pytest.mark.parametrize("n", [1, 97, 333])
@pytest.mark.parametrize("axis", fm.AXES)
def test_exactly_min_deg_k_cells_are_kept_and_the_samples_nest(n, axis):
    src, dst = _graph(n)
    _, _, deg = neighbour_lists(src, dst, n, axis == "col")
    for seed in dm.SEEDS:
        before = None
        for k in (1, 2, 3, 5, 8, 32):
            r, c, keep = fm.kept_mask(src, dst, n, k, seed, axis)
            u = r if axis == "row" else c
            np.testing.assert_array_equal(np.bincount(u[keep], minlength=n), np.minimum(deg, k))
            thr = fm.thresholds(src, dst, n, k, seed, axis)
            assert (thr[deg <= k] == 0).all()
            if before is not None:
                assert (keep | ~before).all(), "the sample for k is a subset of the sample for k + 1 (and of every larger k)"
                assert keep.sum() > before.sum() or (deg <= k).all()
            before = keep
        ks, kd = fm.kept_edges(src, dst, n, 3, seed, axis)
        assert np.isin(ks * n + kd, set_cells(src, dst, n)).all() and np.unique(ks * n + kd).size == ks.size


@pytest.mark.parametrize("axis", fm.AXES)
def test_a_fanout_of_the_largest_degree_keeps_everything(axis):
    n = 333
    src, dst = _graph(n)
    _, _, deg = neighbour_lists(src, dst, n, axis == "col")
    d = int(deg.max())
    for k in (d, d + 1, n):
        assert (fm.thresholds(src, dst, n, k, 1, axis) == 0).all()
        assert fm.kept_mask(src, dst, n, k, 1, axis)[2].all()
    assert (fm.thresholds(src, dst, n, d - 1, 1, axis) != 0).any()


def test_the_two_axes_are_different_samples():
    """A row-axis sample bounds the out-degree only, a column-axis sample the in-degree only: the kept cells differ."""
    n, k, seed = 333, 3, 1
    src, dst = _graph(n)
    rows, cols = fm.kept_mask(src, dst, n, k, seed, "row")[2], fm.kept_mask(src, dst, n, k, seed, "col")[2]
    assert (rows != cols).any()
    r, c, _ = fm.kept_mask(src, dst, n, k, seed, "row")
    assert np.bincount(c[rows], minlength=n).max() > k and np.bincount(r[cols], minlength=n).max() > k
    # ... and the column-axis sample is the row-axis sample of the transposed edge list only up to the hash's coordinates: H is not symmetric
    t = fm.kept_edges(dst, src, n, k, seed, "row")
    kc = fm.kept_edges(src, dst, n, k, seed, "col")
    assert set(zip(t[1].tolist(), t[0].tolist())) != set(zip(kc[0].tolist(), kc[1].tolist()))


def _hash_over_seeds(i, j, seeds):
    """H(i, j, seed) for arrays of cells [d] and seeds [S] -> uint32 [S, d], the model's formula vectorised over the seed"""
    seeds = np.asarray(seeds, dtype=np.uint64)
    k0, k1 = (seeds & np.uint64(0xFFFFFFFF)).astype(np.uint32)[:, None], (seeds >> np.uint64(32)).astype(np.uint32)[:, None]
    i, j = np.asarray(i, dtype=np.uint32)[None, :], np.asarray(j, dtype=np.uint32)[None, :]
    with np.errstate(over="ignore"):
        K = dm.mix32(k0) + k1
        return dm.mix32((dm.mix32(i ^ k0) ^ (dm.mix32(j ^ k1) + dm.GOLDEN)) + K)


SEED_SETS = {"0..4095": np.arange(4096, dtype=np.uint64),
             "multiples of the golden ratio": (np.arange(4096, dtype=np.uint64) * np.uint64(GOLDEN64))}


@pytest.mark.parametrize("seeds", sorted(SEED_SETS))
@pytest.mark.parametrize("d,k,axis", [(8, 3, "row"), (10, 1, "row"), (40, 10, "row"), (8, 3, "col")])
def test_every_neighbour_is_kept_equally_often(d, k, axis, seeds):
    """Keeping the k largest of d distinct pseudo-random keys is a uniform draw without replacement: over 4096 seeds every neighbour's
    keep count is Binomial(4096, k / d) if the hash is good. The bound, 5 standard deviations of that binomial, is derived from it (the
    chance that one of the 66 counts of a seed set exceeds it under the null is below 1e-4) and is no measurement; the seeds are fixed,
    so the outcome is fixed."""
    with np.errstate(over="ignore"):
        S = SEED_SETS[seeds]
    rng = np.random.default_rng(d * 100 + k)
    own, nbrs = 5, np.sort(rng.choice(2000, d, replace=False))
    i, j = (np.full(d, own), nbrs) if axis == "row" else (nbrs, np.full(d, own))
    h = _hash_over_seeds(i, j, S)
    for s in (0, 1, 4095):
        np.testing.assert_array_equal(h[s], dm.H(i, j, int(S[s])))
    kth = np.sort(h, axis=1)[:, d - k]
    counts = (h >= kth[:, None]).sum(axis=0)
    assert counts.sum() == 4096 * k
    p = k / d
    sd = np.sqrt(4096 * p * (1 - p))
    worst = float(np.abs(counts - 4096 * p).max() / sd)
    print(f"d={d} k={k} {axis} {seeds}: worst deviation {worst:.2f} standard deviations")
    assert worst <= 5.0
