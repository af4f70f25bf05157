"""The exact model of the additive edge score (tests/tiled_addscore_model.py) against its float64 dense definition on small graphs, on
both views, and the wrong-rule aids: a fused multiply-add, descending order, the derivative 1 at u = 0 and the butterfly omitted must
each DIFFER from the model on these inputs - otherwise the device comparison, which is bit for bit, would not tell them apart. No GPU."""
import numpy as np
import pytest

import tiled_addscore_model as am
import tiled_esoftmax_model as sm
import tiled_heads_model as hm

F32 = np.float32
SLOPES = (0.0, 0.2, 1.0)


def _case(n, d, seed=0):
    src, dst = sm.graph_edges(n)
    owner, nb, slot, deg = sm.owner_lists(src, dst, n, False)
    rng = np.random.default_rng([n, d, seed])
    own, nbr = rng.normal(size=(n, d)).astype(F32), rng.normal(size=(n, d)).astype(F32)
    att = rng.normal(size=d).astype(F32)
    g = rng.normal(size=slot.size).astype(F32)
    return src, dst, own, nbr, att, g


def force_kinks(src, dst, n, own, nbr):
    """own, nbr with some entries forced so that own + nbr is exactly +0, exactly -0 and negative: for the first cells in slot order,
    column 0 gets x + (-x) = +0, column 1 (where there is one) (-0) + (-0) = -0, the last column a negative sum. A forced entry of a
    node is shared by all its cells; the cells are taken from distinct owners and neighbours."""
    import tiled_edge_model as em

    r, c = em.slot_cells(src, dst, n)
    own, nbr = own.copy(), nbr.copy()
    used_r, used_c, picked = set(), set(), []
    for i, j in zip(r.tolist(), c.tolist()):
        if i not in used_r and j not in used_c and i not in used_c and j not in used_r:
            used_r.add(i)
            used_c.add(j)
            picked.append((i, j))
        if len(picked) == 6:
            break
    d = own.shape[1]
    for t, (i, j) in enumerate(picked):
        for a, b in ((own, nbr), (nbr, own)):   # the same cells on both views
            if t % 3 == 0:
                a[i, 0], b[j, 0] = F32(1.5), F32(-1.5)
            elif t % 3 == 1:
                a[i, min(1, d - 1)], b[j, min(1, d - 1)] = F32(-0.0), F32(-0.0)
            else:
                a[i, d - 1], b[j, d - 1] = F32(-2.0), F32(-0.25)
    return own, nbr


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("n,d", [(33, 5), (129, 70), (300, 8)])
def test_the_model_is_the_float64_definition_up_to_rounding(n, d, transposed):
    src, dst, own, nbr, att, g = _case(n, d)
    own, nbr = force_kinks(src, dst, n, own, nbr)
    deg = sm.owner_degree_per_slot(src, dst, n, transposed).max()
    for slope in SLOPES:
        s = am.addscore_f32(src, dst, n, own, nbr, att, slope, transposed)
        s64 = am.addscore_f64(src, dst, n, own, nbr, att, slope, transposed)
        # every term carries three roundings and the sum of d terms at most d more: |s - s64| <= (d + 3) 2^-24 sum |att L(u)| to first order
        bound = (d + 3) * 2.0 ** -24 * (np.abs(att).astype(np.float64).sum() * 8)
        assert s.dtype == F32 and np.abs(s - s64).max() <= bound
        d_own, P, _ = am.addscore_grad_f32(src, dst, n, own, nbr, att, slope, g, transposed)
        d64, P64 = am.addscore_grad_f64(src, dst, n, own, nbr, att, slope, g, transposed)
        scale = (deg + 3) * 2.0 ** -24 * deg * 64   # a fold of deg terms, each below |g| max|u| <= 64 here
        assert np.abs(d_own - d64).max() <= scale and np.abs(P - P64).max() <= scale


def test_forced_entries_reach_both_zeros_and_the_negative_branch():
    n, d = 129, 5
    src, dst, own, nbr, att, g = _case(n, d)
    own, nbr = force_kinks(src, dst, n, own, nbr)
    owner, nb, _, _ = sm.owner_lists(src, dst, n, False)
    u = own[owner] + nbr[nb]
    bits = u.view(np.uint32)
    assert (bits == 0).any() and (bits == 0x80000000).any() and (u < 0).any() and (u > 0).any()


@pytest.mark.parametrize("transposed", [False, True])
def test_the_wrong_rules_differ_from_the_model(transposed):
    n, d = 300, 70
    src, dst, own, nbr, att, g = _case(n, d, 1)
    own, nbr = force_kinks(src, dst, n, own, nbr)
    slope = 0.2
    s = am.addscore_f32(src, dst, n, own, nbr, att, slope, transposed)
    for wrong in am.SCORE_WRONG:
        w = am.addscore_f32(src, dst, n, own, nbr, att, slope, transposed, wrong=wrong)
        assert (w.view(np.uint32) != s.view(np.uint32)).any(), wrong
        assert np.abs(w - s).max() < 1e-4, wrong   # and yet the same number up to rounding
    d_own, P, FD = am.addscore_grad_f32(src, dst, n, own, nbr, att, slope, g, transposed)
    for wrong in am.GRAD_WRONG:
        wd, wP, _ = am.addscore_grad_f32(src, dst, n, own, nbr, att, slope, g, transposed, wrong=wrong)
        differs = (wd.view(np.uint32) != d_own.view(np.uint32)).any() or (wP.view(np.uint32) != P.view(np.uint32)).any()
        assert differs, wrong
    # the kink alone: at u = +-0 the derivative is the slope, so "kink_one" changes d_own and nothing else
    wd, wP, _ = am.addscore_grad_f32(src, dst, n, own, nbr, att, slope, g, transposed, wrong="kink_one")
    assert (wd != d_own).any() and (wP.view(np.uint32) == P.view(np.uint32)).all()


def test_the_zero_of_u_takes_the_slope_whatever_its_sign():
    src, dst = np.array([0, 0]), np.array([1, 2])
    own = np.array([[1.5, -0.0], [0, 0], [0, 0]], dtype=F32)
    nbr = np.array([[0, 0], [-1.5, -0.0], [7.0, 7.0]], dtype=F32)   # cell (0, 1): u = (+0, -0); cell (0, 2): u > 0
    att = np.array([2.0, 3.0], dtype=F32)
    g = np.array([1.0, 10.0], dtype=F32)
    d_own, P, FD = am.addscore_grad_f32(src, dst, 3, own, nbr, att, 0.25, g)
    assert FD[0].tolist() == [10.25, 10.25] and d_own[0].tolist() == [20.5, 30.75]
    assert P[0].tolist() == [85.0, 70.0]   # 1 * L(+-0) + 10 * 8.5, 10 * 7
    s = am.addscore_f32(src, dst, 3, own, nbr, att, 0.25)
    assert s.tolist() == [0.0, 2.0 * 8.5 + 3.0 * 7.0]


def test_heads_are_the_single_head_model_on_slices():
    n, H, d = 33, 3, 5
    src, dst, own, nbr, att, _ = _case(n, H * d, 2)
    nnz = sm.owner_lists(src, dst, n, False)[2].size
    g = np.random.default_rng(3).normal(size=(nnz, H)).astype(F32)
    s = am.addscore_heads_f32(src, dst, n, own, nbr, att.reshape(H, d), 0.2, H)
    d_own, P = am.addscore_grad_heads_f32(src, dst, n, own, nbr, att, 0.2, g, H, True)
    for h in range(H):
        c = hm.head_cols(h, d)
        assert (s[:, h] == am.addscore_f32(src, dst, n, own[:, c], nbr[:, c], att[c], 0.2)).all()
        one = am.addscore_grad_f32(src, dst, n, own[:, c], nbr[:, c], att[c], 0.2, g[:, h], True)
        assert (d_own[:, c] == one[0]).all() and (P[:, c] == one[1]).all()


def test_an_owner_without_cells_and_a_graph_without_cells():
    src, dst, own, nbr, att, g = _case(33, 4, 4)
    for transposed, lonely in ((False, 5), (True, 9)):   # row 5 and column 9 have no edges
        d_own, P, FD = am.addscore_grad_f32(src, dst, 33, own, nbr, np.abs(att), 0.2, g, transposed)
        assert (FD[lonely].view(np.uint32) == 0).all() and (P[lonely].view(np.uint32) == 0).all() and (d_own[lonely].view(np.uint32) == 0).all()
    none = np.zeros(0, dtype=np.int64)
    d_own, P, _ = am.addscore_grad_f32(none, none, 3, own[:3], nbr[:3], -np.abs(att), 0.2, np.zeros(0, dtype=F32))
    assert (d_own.view(np.uint32) == 0).all() and (P.view(np.uint32) == 0).all()
    assert am.addscore_f32(none, none, 3, own[:3], nbr[:3], att, 0.2).shape == (0,)
