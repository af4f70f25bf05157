"""Exact NumPy model of the additive edge score of the tiled adjacency and its gradients (include/qgtc_addscore.h;
tiled.tiledEdgeAdditiveScores / tiledEdgeAdditiveAttention, conv.GATv2Conv), for ONE head: heads are per-slice applications of it, as in
tests/tiled_heads_model.py. It stands on tests/tiled_edge_model.py's slot order and tests/tiled_esoftmax_model.py's owner lists (an
owner's cells by ascending neighbour id). Every operation is one np.float32 operation in the order the header fixes, so the results are
compared with the device's bit for bit. The float64 functions beside them are the definitions the model is held against. No GPU."""
import numpy as np

import tiled_edge_model as em
import tiled_esoftmax_model as sm
from tiled_attn_model import _fold, lrelu_f32

F32 = np.float32

SCORE_WRONG = ("fma", "no_butterfly")
GRAD_WRONG = ("fma", "descending", "kink_one")


def addscore_rows_f32(x, y, att, slope, wrong=None):
    """ADDSCORE of the header for every row pair of x, y [R, d] with att [d]: 64 in-order partial sums of fl(att[c] * L(fl(x + y))) over
    the columns j, j + 64, ..., then the six exchange steps; float32 [R]. `wrong`: "fma" rounds att * L(u) + t once, "no_butterfly" adds
    the 64 partial sums in lane order instead (WRONG rules, test aids)."""
    assert wrong in (None,) + SCORE_WRONG
    x, y, att = (np.ascontiguousarray(t, dtype=F32) for t in (x, y, att))
    assert x.ndim == 2 and x.shape == y.shape and att.shape == (x.shape[1],)
    R, d = x.shape
    t = np.zeros((R, 64), dtype=F32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for c in range(0, d, 64):
            w = min(64, d - c)
            lu = lrelu_f32(x[:, c:c + w] + y[:, c:c + w], slope)
            if wrong == "fma":
                t[:, :w] = (t[:, :w].astype(np.float64) + att[None, c:c + w].astype(np.float64) * lu.astype(np.float64)).astype(F32)
            else:
                t[:, :w] = t[:, :w] + att[None, c:c + w] * lu
        if wrong == "no_butterfly":
            s = np.zeros(R, dtype=F32)
            for j in range(64):
                s = s + t[:, j]
            return s
        lane = np.arange(64)
        for h in (32, 16, 8, 4, 2, 1):
            t = t + t[:, lane ^ h]
    assert t.dtype == F32 and (t.view(np.uint32) == t[:, :1].view(np.uint32)).all()
    return t[:, 0].copy()


def addscore_f32(src, dst, n, own, nbr, att, slope, transposed=False, wrong=None):
    """float32 [nnz] in slot order: ADDSCORE(own[o], nbr[k]; att) for the stored cell with owner o and neighbour k on the view"""
    r, c = em.slot_cells(src, dst, n)
    own, nbr = np.ascontiguousarray(own, dtype=F32), np.ascontiguousarray(nbr, dtype=F32)
    if r.size == 0:
        return np.zeros(0, dtype=F32)
    o, k = (c, r) if transposed else (r, c)
    return addscore_rows_f32(own[o], nbr[k], att, slope, wrong)


def addscore_grad_f32(src, dst, n, own, nbr, att, slope, g, transposed=False, wrong=None):
    """(d_own, P, FD) float32 [n, d] each, for the owners of the view: the two in-order folds over an owner's cells by ascending
    neighbour id, d_own = fl(att * FD), P = FV. An adjacency without cells gives +0 everywhere (the entry's rule). `wrong`: "fma" rounds
    g * L(u) + acc once, "descending" folds from the highest id down, "kink_one" takes the derivative 1 at u = 0 (WRONG rules)."""
    assert wrong in (None,) + GRAD_WRONG
    own, nbr, att, g = (np.ascontiguousarray(t, dtype=F32) for t in (own, nbr, att, g))
    owner, nb, slot, deg = sm.owner_lists(src, dst, n, transposed, wrong == "descending")
    assert g.shape == (slot.size,) and own.shape == nbr.shape and att.shape == (own.shape[1],)
    if slot.size == 0:
        z = np.zeros_like(own)
        return z, z.copy(), z.copy()
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        u = own[owner] + nbr[nb]
        gk = g[slot][:, None]
        live = u >= 0 if wrong == "kink_one" else u > 0
        T = np.where(live, gk, F32(slope) * gk).astype(F32)
        FD = _fold(n, owner, T)
        lu = lrelu_f32(u, slope)
        if wrong == "fma":
            start = np.concatenate([[0], np.cumsum(deg)[:-1]])
            FV = np.zeros_like(own)
            for k in range(int(deg.max())):
                rows = np.flatnonzero(deg > k)
                pos = start[rows] + k
                FV[rows] = (FV[rows].astype(np.float64) + gk[pos].astype(np.float64) * lu[pos].astype(np.float64)).astype(F32)
        else:
            FV = _fold(n, owner, (gk * lu).astype(F32))
        d_own = att[None, :] * FD
    assert d_own.dtype == F32 and FV.dtype == F32 and FD.dtype == F32
    return d_own, FV, FD


# ---- heads: the single-head model per contiguous slice -------------------------------------------------------------------------------------
def _cols(h, d):
    return slice(h * d, (h + 1) * d)


def addscore_heads_f32(src, dst, n, own, nbr, att, slope, heads, transposed=False):
    """float32 [nnz, H]: column h is addscore_f32 on head h's columns of own, nbr and att (att is [N] or [H, d])"""
    own, nbr = np.ascontiguousarray(own, dtype=F32), np.ascontiguousarray(nbr, dtype=F32)
    att = np.ascontiguousarray(att, dtype=F32).reshape(-1)
    d = own.shape[1] // heads
    cols = [addscore_f32(src, dst, n, own[:, _cols(h, d)], nbr[:, _cols(h, d)], att[_cols(h, d)], slope, transposed) for h in range(heads)]
    return np.ascontiguousarray(np.stack(cols, axis=1), dtype=F32)


def addscore_grad_heads_f32(src, dst, n, own, nbr, att, slope, g, heads, transposed=False):
    """(d_own, P) float32 [n, N]: head h's columns are addscore_grad_f32 on head h's columns with the gradient g[:, h]"""
    own, nbr = np.ascontiguousarray(own, dtype=F32), np.ascontiguousarray(nbr, dtype=F32)
    att = np.ascontiguousarray(att, dtype=F32).reshape(-1)
    g = np.ascontiguousarray(g, dtype=F32).reshape(-1, heads)
    d = own.shape[1] // heads
    d_own, P = np.zeros_like(own), np.zeros_like(own)
    for h in range(heads):
        c = _cols(h, d)
        d_own[:, c], P[:, c], _ = addscore_grad_f32(src, dst, n, own[:, c], nbr[:, c], att[c], slope, g[:, h], transposed)
    return d_own, P


def additive_attention_heads_f32(src, dst, n, own, nbr, V, att, slope, heads, transposed=False):
    """(out float32 [n, Nv], scores [nnz, H], alpha [nnz, H]): the models composed as tiledEdgeAdditiveAttention composes the launches"""
    import tiled_heads_model as hm

    s = addscore_heads_f32(src, dst, n, own, nbr, att, slope, heads, transposed)
    alpha = hm.edge_softmax_heads_f32(src, dst, n, s, transposed)[0]
    return hm.weighted_heads_f32(src, dst, n, V, alpha, transposed), s, alpha


def additive_attention_grads_heads_f32(src, dst, n, own, nbr, V, att, slope, heads, dY, transposed=False):
    """(d_own, d_nbr, dV, P) float32 for the incoming gradient dY, composed as autograd composes the launches: dV = the weighted sum on
    the other view, dalpha = SDDMM(dY, V), dscores = the softmax gradient, then the two gradient launches of the score; att's gradient
    is the column sum of P, which is the caller's reduction."""
    import tiled_heads_model as hm

    _, _, alpha = additive_attention_heads_f32(src, dst, n, own, nbr, V, att, slope, heads, transposed)
    dV = hm.weighted_heads_f32(src, dst, n, dY, alpha, not transposed)
    dalpha = hm.sddmm_heads_f32(src, dst, n, dY, V, heads, transposed)
    ds = hm.edge_softmax_grad_heads_f32(src, dst, n, alpha, dalpha, transposed)
    d_own, P = addscore_grad_heads_f32(src, dst, n, own, nbr, att, slope, ds, heads, transposed)
    d_nbr, _ = addscore_grad_heads_f32(src, dst, n, nbr, own, att, slope, ds, heads, not transposed)
    return d_own, d_nbr, dV, P


# ---- the float64 definitions ----------------------------------------------------------------------------------------------------------------
def addscore_f64(src, dst, n, own, nbr, att, slope, transposed=False):
    r, c = em.slot_cells(src, dst, n)
    o, k = (c, r) if transposed else (r, c)
    u = np.asarray(own, dtype=np.float64)[o] + np.asarray(nbr, dtype=np.float64)[k]
    return (np.where(u > 0, u, slope * u) * np.asarray(att, dtype=np.float64)[None, :]).sum(axis=1)


def addscore_grad_f64(src, dst, n, own, nbr, att, slope, g, transposed=False):
    """(d_own, P) float64 [n, d]; the derivative at u = 0 is the slope"""
    r, c = em.slot_cells(src, dst, n)
    o, k = (c, r) if transposed else (r, c)
    u = np.asarray(own, dtype=np.float64)[o] + np.asarray(nbr, dtype=np.float64)[k]
    gk = np.asarray(g, dtype=np.float64)[:, None]
    FD, FV = np.zeros((n, u.shape[1])), np.zeros((n, u.shape[1]))
    np.add.at(FD, o, np.where(u > 0, gk, slope * gk))
    np.add.at(FV, o, gk * np.where(u > 0, u, slope * u))
    return np.asarray(att, dtype=np.float64)[None, :] * FD, FV
