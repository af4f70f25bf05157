"""The edge-dropout rule (include/qgtc.h, "Edge dropout") as tests/tiled_drop_model.py states it: known answers of the hash, the
thresholds, the host function qgtc_edge_kept against the model, the statistics of the mask (kept fraction, independence of the
transpose, of other seeds and of the row / column permutations a weaker combine would reduce a seed change to), the wrong rules, and
masking = dropping in the models. No GPU."""
import itertools

import numpy as np
import pytest

import tiled_drop_model as dm
from tiled_attn_model import attention_f32
from tiled_float_model import aggregate_f32, neighbour_lists
from tiled_max_model import MAX, MIN, extremum_f32
from tiled_model import random_edges, set_cells

KAT_CELLS = ((0, 0), (1, 0), (5, 7), (1000, 999), (8388607, 8388607))
KAT = {
    0: "01fce552 5dd09b26 fef076a7 a56f4a80 9b01f9c2",
    1: "a263e079 b21c8e52 5cb9f6d8 1b063cf8 48c38ddf",
    0x0123456789ABCDEF: "403f6c8a 0f7219b6 a9a10bec 825be890 24dfb64d",
    2 ** 64 - 1: "d39d7ce6 7358fe55 4ae81848 1b08b3ba 9daa3433",
}
GRID = 2048
GRID_SEEDS = (0, 1, 2 ** 32, 2 ** 64 - 1)
RATES = (0.1, 0.5, 0.6)


def test_known_answers():
    assert int(dm.mix32(1)) == 0x688990C0
    assert tuple(KAT) == dm.SEEDS
    for seed, words in KAT.items():
        got = " ".join("%08x" % int(dm.H(i, j, seed)) for i, j in KAT_CELLS)
        assert got == words, hex(seed)
        i, j = np.array(KAT_CELLS).T          # the vector path gives the same words
        assert [int(h) for h in dm.H(i, j, seed)] == [int(w, 16) for w in words.split()]


def test_thresholds():
    assert dm.threshold(0.0) == 0
    assert dm.threshold(0.1) == 429496729
    assert dm.threshold(0.6) == 2576980377
    assert dm.threshold(1.0 - 2.0 ** -32) == 2 ** 32 - 1
    for T in (1, 12345, 2 ** 31, 2 ** 32 - 1):   # T / 2^32 is a double, and comes back as T: any threshold can be asked for as a rate
        assert dm.threshold(T / 2.0 ** 32) == T


@pytest.fixture(scope="module")
def edge_kept():
    from qgtc_ppopp22_amd import cabi

    return cabi.load().qgtc_edge_kept


def test_host_function_equals_the_model(edge_kept):
    rng = np.random.default_rng(11)
    per_seed = 25000                               # 10^5 cells over the four seeds
    for seed in dm.SEEDS:
        i = rng.integers(0, 2 ** 23, size=per_seed)
        j = rng.integers(0, 2 ** 23, size=per_seed)
        i[:4], j[:4] = (0, 2 ** 23 - 1, 0, 2 ** 23 - 1), (0, 0, 2 ** 23 - 1, 2 ** 23 - 1)
        T = rng.integers(0, 2 ** 32, size=per_seed)
        T[:3] = (0, 2 ** 32 - 1, dm.threshold(0.5))
        h = dm.H(i, j, seed)
        T[3:40] = h[3:40].astype(np.int64)         # on the boundary: H == T is kept
        T[40:80] = np.minimum(h[40:80].astype(np.int64) + 1, 2 ** 32 - 1)
        want = h >= T.astype(np.uint32)
        got = np.array([edge_kept(int(a), int(b), seed, int(t)) for a, b, t in zip(i, j, T)], dtype=bool)
        assert (got == want).all(), hex(seed)
        assert want[3:40].all()


@pytest.fixture(scope="module")
def grid_hashes():
    i, j = np.meshgrid(np.arange(GRID), np.arange(GRID), indexing="ij")
    return {seed: dm.H(i, j, seed) for seed in GRID_SEEDS}


def _corr(a, b):
    a, b = a.ravel().astype(np.float64), b.ravel().astype(np.float64)
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


def test_mask_statistics(grid_hashes):
    cells = GRID * GRID
    idx = np.arange(GRID)
    worst_sd = worst_t = worst_pair = 0.0
    for rate in RATES:
        T = np.uint32(dm.threshold(rate))
        masks = {seed: h >= T for seed, h in grid_hashes.items()}
        for seed, m in masks.items():
            sd = abs(m.mean() - (1.0 - rate)) / np.sqrt(rate * (1.0 - rate) / cells)
            worst_sd = max(worst_sd, sd)
            assert sd < 4.0, (rate, hex(seed), sd)
            c = abs(_corr(m, m.T))
            worst_t = max(worst_t, c)
            assert c < 0.01, (rate, hex(seed), c)
        for a, b in itertools.combinations(GRID_SEEDS, 2):
            ma, mb = masks[a], masks[b]
            d0, d1 = (a ^ b) & 0xFFFFFFFF, (a ^ b) >> 32
            # a combine without K reduces a change of one seed word to a permutation of the rows (i ^ d0) or the columns (j ^ d1)
            variants = [("as is", mb)]
            if 0 < d0 < GRID:
                variants.append(("rows", mb[idx ^ d0, :]))
            if 0 < d1 < GRID:
                variants.append(("columns", mb[:, idx ^ d1]))
            if 0 < d0 < GRID and 0 < d1 < GRID:
                variants.append(("both", mb[idx ^ d0, :][:, idx ^ d1]))
            for name, v in variants:
                assert (ma != v).any(), (rate, hex(a), hex(b), name)
                c = abs(_corr(ma, v))
                worst_pair = max(worst_pair, c)
                assert c < 0.01, (rate, hex(a), hex(b), name, c)
    print(f"kept fraction: worst {worst_sd:.2f} sd; |corr| with the transpose <= {worst_t:.4f}; across seeds <= {worst_pair:.4f}")


def test_the_weaker_combine_is_caught(grid_hashes):
    """Without K the statistics above fail: seeds 0 and 1 give the same mask with the rows permuted."""
    i, j = np.meshgrid(np.arange(GRID), np.arange(GRID), indexing="ij")
    T = np.uint32(dm.threshold(0.5))
    m0, m1 = dm.H(i, j, 0, wrong="no_K") >= T, dm.H(i, j, 1, wrong="no_K") >= T
    assert (m0 == m1[np.arange(GRID) ^ 1, :]).all()


GRAPHS = [(97, 400, 1), (333, 1500, 2), (1000, 4000, 3)]


@pytest.mark.parametrize("n,e,gseed", GRAPHS)
def test_every_wrong_rule_differs_on_the_test_graphs(n, e, gseed):
    src, dst = random_edges(np.random.default_rng(gseed), n, e)
    cells = set_cells(src, dst, n)
    r, c = cells // n, cells % n
    T = dm.threshold(0.6)
    for seed in dm.SEEDS:
        right = dm.kept(r, c, seed, T)
        for wrong in ("transposed", "swapped_seed", "no_K"):
            differs = (dm.kept(r, c, seed, T, wrong) != right).any()
            if wrong == "swapped_seed" and (seed & 0xFFFFFFFF) == seed >> 32:
                assert not differs                  # seeds 0 and 2^64 - 1 have equal words: swapping them changes nothing
            elif wrong == "no_K" and seed == 0:
                assert not differs                  # K(0) = mix32(0) + 0 = 0: leaving it out changes nothing
            else:
                assert differs, (wrong, hex(seed))
        # ">" differs only on the boundary: a threshold equal to a cell's hash (any threshold is a rate: T / 2^32)
        Tb = int(dm.H(r[0], c[0], seed))
        assert dm.kept(r[0], c[0], seed, Tb) and not dm.kept(r[0], c[0], seed, Tb, ">")


def _masked_loops(src, dst, n, X, T, seed, transposed):
    """sum, max and arg by plain loops over the UNFILTERED neighbour lists with the keep test inside: masking, not dropping"""
    out_row, nb, _ = neighbour_lists(src, dst, n, transposed)
    s = np.zeros(X.shape, dtype=np.float32)
    mx = np.zeros(X.shape, dtype=np.float32)
    arg = np.full(X.shape, -1, dtype=np.int32)
    for o, v in zip(out_row, nb):
        i, j = (v, o) if transposed else (o, v)     # the cell is A's on either view
        if not dm.kept(i, j, seed, T):
            continue
        s[o] = s[o] + X[v]
        take = (arg[o] < 0) | (X[v] > mx[o])
        mx[o] = np.where(take, X[v], mx[o])
        arg[o] = np.where(take, v, arg[o])
    return s, mx, arg


@pytest.mark.parametrize("transposed", [False, True])
def test_masking_equals_dropping_in_the_models(transposed):
    n, N = 97, 5
    rng = np.random.default_rng(5)
    src, dst = random_edges(rng, n, 500)
    X = rng.standard_normal((n, N)).astype(np.float32)
    for seed, rate in ((1, 0.1), (2 ** 64 - 1, 0.6), (0x0123456789ABCDEF, 0.0)):
        T = dm.threshold(rate)
        ks, kd = dm.kept_edges(src, dst, n, T, seed)
        s, mx, arg = _masked_loops(src, dst, n, X, T, seed, transposed)
        assert (aggregate_f32(ks, kd, n, X, transposed).view(np.uint32) == s.view(np.uint32)).all()
        m_out, m_arg = extremum_f32(ks, kd, n, X, transposed, MAX)
        assert (m_out.view(np.uint32) == mx.view(np.uint32)).all() and (m_arg == arg).all()
        if rate == 0.0:                             # rate 0 keeps the whole graph
            assert ks.size == set_cells(src, dst, n).size
            assert (aggregate_f32(src, dst, n, X, transposed).view(np.uint32) == s.view(np.uint32)).all()
    # the attention model on the kept edges against a float64 masked softmax over the dense adjacency
    seed, T = 7, dm.threshold(0.5)
    p, q = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    ks, kd = dm.kept_edges(src, dst, n, T, seed)
    out, m, inv = attention_f32(ks, kd, n, X, p, q, 0.2, transposed)
    A = np.zeros((n, n), dtype=bool)
    cells = set_cells(src, dst, n)
    A[cells // n, cells % n] = True
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    A &= dm.kept(i, j, seed, T)
    if transposed:
        A = A.T
    e = p[:, None].astype(np.float64) + q[None, :].astype(np.float64)
    e = np.where(A, np.where(e > 0, e, 0.2 * e), -np.inf)
    has = A.any(axis=1)
    w = np.where(A, np.exp(e - np.where(has, e.max(axis=1), 0.0)[:, None]), 0.0)
    ref = np.where(has[:, None], (w / np.where(has, w.sum(axis=1), 1.0)[:, None]) @ X.astype(np.float64), 0.0)
    assert np.allclose(out, ref, rtol=1e-5, atol=1e-6)
    assert (inv[~has] == 0).all() and (out[~has] == 0).all()


def test_min_of_the_kept_edges_is_the_masked_min():
    n, N = 97, 3
    rng = np.random.default_rng(9)
    src, dst = random_edges(rng, n, 500)
    X = rng.standard_normal((n, N)).astype(np.float32)
    T, seed = dm.threshold(0.6), 1
    ks, kd = dm.kept_edges(src, dst, n, T, seed)
    out, arg = extremum_f32(ks, kd, n, X, False, MIN)
    _, neg_max, neg_arg = _masked_loops(src, dst, n, -X, T, seed, False)
    assert (out == -neg_max).all() and (arg == neg_arg).all()
