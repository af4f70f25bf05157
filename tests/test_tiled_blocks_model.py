"""tests/tiled_blocks_model.py against the definitions it models (include/qgtc_blocks.h), without a GPU: a masked sample is the unmasked
sample of the re-packed induced edge list, counts are min(deg_m, k), the frontier is the set of neighbour ends of the kept edges, a chain
of blocks is nested, and two all-ones masks give tests/tiled_fanout_model.py."""
import numpy as np
import pytest

import tiled_blocks_model as bm
import tiled_fanout_model as fm
from tiled_drop_model import SEEDS
from tiled_model import random_edges

CASES = [(n, k) for n in (1, 97, 333) for k in (1, 3, 8)]


def _graph(n, seed=0):
    rng = np.random.default_rng(100 * n + seed)
    src, dst = random_edges(rng, n, 6 * n + 5)
    return rng, src, dst, np.arange(n) % 3 == 0, rng.random(n) < 0.5


@pytest.mark.parametrize("n,k", CASES)
@pytest.mark.parametrize("axis", fm.AXES)
def test_the_masked_sample_is_the_sample_of_the_repacked_induced_edges(n, k, axis):
    _, src, dst, row, nbr = _graph(n)
    for seed in SEEDS[:2]:
        for r, b in ((row, nbr), (row, None), (None, nbr)):
            isrc, idst = bm.induced_edges(src, dst, n, axis, r, b)
            thr, kept = bm.thresholds_counts(src, dst, n, k, seed, axis, r, b)
            np.testing.assert_array_equal(thr, fm.thresholds(isrc, idst, n, k, seed, axis))
            deg = bm.degrees_masked(src, dst, n, axis, r, b)
            np.testing.assert_array_equal(kept, np.minimum(deg, k))
            ks, kd = bm.kept_edges(src, dst, n, k, seed, axis, r, b)
            ws, wd = fm.kept_edges(isrc, idst, n, k, seed, axis)
            np.testing.assert_array_equal(ks, ws)
            np.testing.assert_array_equal(kd, wd)
            np.testing.assert_array_equal(np.bincount(ks if axis == "row" else kd, minlength=n), kept)   # exactly kept[u] cells per node
            if r is not None:
                assert not thr[~r].any() and not kept[~r].any()
            front = bm.frontier(src, dst, n, k, seed, axis, r, b)
            np.testing.assert_array_equal(np.nonzero(front)[0], np.unique(wd if axis == "row" else ws))
            if b is not None:
                assert not (front & ~b).any()


@pytest.mark.parametrize("axis", fm.AXES)
def test_all_ones_masks_give_the_unmasked_model(axis):
    n, k, seed = 333, 3, SEEDS[1]
    _, src, dst, _, _ = _graph(n)
    ones = np.ones(n, dtype=bool)
    want = fm.thresholds(src, dst, n, k, seed, axis)
    for r, b in ((None, None), (ones, ones), (ones, None)):
        np.testing.assert_array_equal(bm.thresholds_counts(src, dst, n, k, seed, axis, r, b)[0], want)
        for got, w in zip(bm.kept_edges(src, dst, n, k, seed, axis, r, b), fm.kept_edges(src, dst, n, k, seed, axis)):
            np.testing.assert_array_equal(got, w)


def test_bitmaps_round_trip_with_zero_pad_bits():
    rng = np.random.default_rng(1)
    for n in (1, 31, 32, 33, 127, 128, 129, 1000):
        flags = rng.random(n) < 0.5
        words = bm.bitmap(flags)
        assert words.dtype == np.int32 and words.shape == (bm.words_of(n),)
        np.testing.assert_array_equal(bm.flags_of(words, n), flags)
        for i in np.nonzero(flags)[0][:5]:
            assert (int(words.view(np.uint32)[i >> 5]) >> (31 - (i & 31))) & 1
    with pytest.raises(AssertionError, match="pad bits"):
        bm.flags_of(np.full(4, -1, dtype=np.int32), 100)


@pytest.mark.parametrize("axis", fm.AXES)
def test_a_chain_of_blocks_is_nested(axis):
    n, fanouts, seed = 1000, (3, 2), 5
    rng, src, dst, _, _ = _graph(n)
    seeds = np.zeros(n, dtype=bool)
    seeds[rng.permutation(n)[:20]] = True
    chain = bm.blocks(src, dst, n, axis, seeds, fanouts, seed)
    assert len(chain) == 2 and (chain[-1]["rows"] == seeds).all()
    assert chain[1]["seed"] == seed and chain[0]["seed"] == (seed + bm.GOLDEN64) % (1 << 64)
    assert [b["k"] for b in chain] == list(fanouts)
    for l, b in enumerate(chain):
        assert not (b["rows"] & ~b["inputs"]).any()                    # a layer's inputs contain its outputs
        if l + 1 < len(chain):
            assert not (chain[l + 1]["rows"] & ~b["rows"]).any()       # rows_{l+1} is a subset of rows_l
        if l:
            assert (chain[l - 1]["rows"] == b["inputs"]).all()          # the next hop samples this hop's inputs
        ks, kd = bm.kept_edges(src, dst, n, b["k"], b["seed"], axis, b["rows"])
        u, v = (ks, kd) if axis == "row" else (kd, ks)
        assert b["rows"][u].all() and b["inputs"][v].all()             # the kept neighbours are a subset of inputs
        np.testing.assert_array_equal(b["kept"], np.minimum(bm.degrees_masked(src, dst, n, axis, b["rows"]), b["k"]))
    sizes = [int(b["rows"].sum()) for b in chain] + [int(chain[0]["inputs"].sum())]
    assert 20 == sizes[1] < sizes[0] < sizes[2] < n, sizes             # the batch grows hop by hop and stays a mini-batch
