"""Exact NumPy model of the edge softmax of the tiled adjacency (include/qgtc.h, "Edge softmax"; tiled.tiledEdgeSoftmax and its gradient
on adj and adj.T, tiled.tiledEdgeScores, tiled.tiledEdgeAttention), on top of tests/tiled_edge_model.py's slot lists and
tests/tiled_attn_model.py's EXP and in-order fold. Every operation is one np.float32 operation in the order the header fixes, so the
results are compared with the device's bit for bit. The float64 functions beside them are the definitions the model is held against.
No GPU."""
import numpy as np

import tiled_edge_model as em
from tiled_attn_model import _fold, exp_f32
from tiled_model import random_edges

F32 = np.float32

FORWARD_WRONG = ("descending", "divide")
GRAD_WRONG = ("descending", "fma")


def graph_edges(n):
    """The edge list of tests/test_tiled_edge_gpu.py's graph on n nodes: random edges (some doubled, which unsets the cell); at n = 300
    a hub column (node 7 adjacent to every row), one full tile (rows 32 .. 63 x columns 128 .. 255), and from n = 33 on row 5 and
    column 9 without edges."""
    rng = np.random.default_rng(100 + n)
    src, dst = (np.asarray(a, dtype=np.int64) for a in random_edges(rng, n, max(4, 4 * n)))
    if n == 300:
        every = np.arange(n)
        full_r, full_c = np.meshgrid(np.arange(32, 64), np.arange(128, 256), indexing="ij")
        keep = (dst != 7) & ~((src >= 32) & (src < 64) & (dst >= 128) & (dst < 256))
        src, dst = src[keep], dst[keep]
        src = np.concatenate([src, every, full_r.ravel()])
        dst = np.concatenate([dst, np.full(n, 7), full_c.ravel()])
    if n >= 33:
        keep = (src != 5) & (dst != 9)
        src, dst = src[keep], dst[keep]
    return src, dst


def owner_lists(src, dst, n, transposed, descending=False):
    """(owner, other end, slot) of the stored cells sorted by (owner, other end ascending - or descending, a WRONG order), and every
    owner's number of cells"""
    owner, nb, slot, deg = em._lists(src, dst, n, transposed)
    if descending:
        order = np.lexsort((-nb, owner))
        owner, nb, slot = owner[order], nb[order], slot[order]
    return owner, nb, slot, deg


def _first_max(n, owner, deg, l):
    """m[o] = l_1, then m = l_k > m ? l_k : m over o's cells in list order; +0 for an owner without cells"""
    start = np.concatenate([[0], np.cumsum(deg)[:-1]])
    m = np.zeros(n, dtype=F32)
    with np.errstate(invalid="ignore"):
        for k in range(int(deg.max()) if deg.size and l.size else 0):
            rows = np.flatnonzero(deg > k)
            lk = l[start[rows] + k]
            m[rows] = lk if k == 0 else np.where(lk > m[rows], lk, m[rows])
    return m


def edge_softmax_f32(src, dst, n, logits, transposed=False, wrong=None):
    """(alpha float32 [nnz] in slot order, m float32 [n], inv float32 [n]) of the forward. `wrong` names a WRONG rule, a test aid:
    "descending" takes an owner's cells from the highest id down, "divide" writes w / den instead of w * inv."""
    assert wrong in (None,) + FORWARD_WRONG
    logits = np.ascontiguousarray(logits, dtype=F32)
    owner, _, slot, deg = owner_lists(src, dst, n, transposed, wrong == "descending")
    assert logits.shape == (slot.size,)
    with np.errstate(all="ignore"):
        l = logits[slot]
        m = _first_max(n, owner, deg, l)
        w = exp_f32(l - m[owner])
        den = _fold(n, owner, w)
        inv = np.where(den > 0, F32(1) / den, F32(0)).astype(F32)
        a = w / den[owner] if wrong == "divide" else w * inv[owner]
    alpha = np.zeros(slot.size, dtype=F32)
    alpha[slot] = a
    assert alpha.dtype == F32 and m.dtype == F32 and inv.dtype == F32
    return alpha, m, inv


def edge_softmax_grad_f32(src, dst, n, alpha, g, transposed=False, wrong=None):
    """float32 [nnz] in slot order: alpha_k * (g_k - S[o]) with S the in-order fold of fl(alpha * g). `wrong`: "descending" folds from
    the highest id down, "fma" rounds alpha * g + S once."""
    assert wrong in (None,) + GRAD_WRONG
    alpha, g = np.ascontiguousarray(alpha, dtype=F32), np.ascontiguousarray(g, dtype=F32)
    owner, _, slot, deg = owner_lists(src, dst, n, transposed, wrong == "descending")
    assert alpha.shape == (slot.size,) and g.shape == alpha.shape
    with np.errstate(all="ignore"):
        a, gg = alpha[slot], g[slot]
        if wrong == "fma":
            start = np.concatenate([[0], np.cumsum(deg)[:-1]])
            S = np.zeros(n, dtype=F32)
            for k in range(int(deg.max()) if deg.size and a.size else 0):
                rows = np.flatnonzero(deg > k)
                pos = start[rows] + k
                S[rows] = (S[rows].astype(np.float64) + a[pos].astype(np.float64) * gg[pos].astype(np.float64)).astype(F32)
        else:
            S = _fold(n, owner, a * gg)
        o = a * (gg - S[owner])
    out = np.zeros(slot.size, dtype=F32)
    out[slot] = o
    assert out.dtype == F32
    return out


def edge_softmax_f64(src, dst, n, logits, transposed=False):
    """float64 [nnz]: the definition, exp(l - max) / sum per owner (finite logits)"""
    owner, _, slot, _ = owner_lists(src, dst, n, transposed)
    l = np.asarray(logits, dtype=np.float64)[slot]
    mx = np.full(n, -np.inf)
    np.maximum.at(mx, owner, l)
    w = np.exp(l - mx[owner])
    den = np.bincount(owner, weights=w, minlength=n)
    out = np.zeros(slot.size)
    out[slot] = w / den[owner]
    return out


def edge_softmax_grad_f64(src, dst, n, alpha, g, transposed=False):
    """float64 [nnz]: alpha * (g - sum over the owner's cells of alpha * g)"""
    owner, _, slot, _ = owner_lists(src, dst, n, transposed)
    a, gg = np.asarray(alpha, dtype=np.float64)[slot], np.asarray(g, dtype=np.float64)[slot]
    S = np.bincount(owner, weights=a * gg, minlength=n)
    out = np.zeros(slot.size)
    out[slot] = a * (gg - S[owner])
    return out


def owner_degree_per_slot(src, dst, n, transposed=False):
    """int64 [nnz]: the number of cells of each slot's owner (the length of the folds behind that slot's value)"""
    owner, _, slot, deg = owner_lists(src, dst, n, transposed)
    out = np.zeros(slot.size, dtype=np.int64)
    out[slot] = deg[owner]
    return out


def pair_logits(src, dst, n, p, q, slope, transposed=False):
    """float32 [nnz] in slot order: L(fl(p[owner] + q[other end])), the logits that attn=(p, q) rebuilds inside its tile walk"""
    from tiled_attn_model import lrelu_f32

    owner, nb, slot, _ = owner_lists(src, dst, n, transposed)
    p, q = np.asarray(p, dtype=F32), np.asarray(q, dtype=F32)
    out = np.zeros(slot.size, dtype=F32)
    out[slot] = lrelu_f32(p[owner] + q[nb], slope)
    return out


def edge_attention_f32(src, dst, n, Q, K, V, scale, transposed=False):
    """(out float32 [n, N], logits, alpha): the model's pieces composed as tiledEdgeAttention composes the launches - the SDDMM, one
    float32 multiply by float32(scale) per slot, the edge softmax, the weighted sum."""
    s = em.sddmm_f32(src, dst, n, Q, K, transposed)
    logits = (s * F32(scale)).astype(F32)
    alpha, _, _ = edge_softmax_f32(src, dst, n, logits, transposed)
    return em.weighted_f32(src, dst, n, V, alpha, transposed), logits, alpha


def edge_attention_grads_f32(src, dst, n, Q, K, V, scale, dY, transposed=False):
    """(dQ, dK, dV) float32 of edge_attention_f32 for the incoming gradient dY, composed as autograd composes the launches:
    dV = the weighted sum on the other view, dalpha = SDDMM(dY, V), dlogits = the softmax gradient, ds = dlogits * scale,
    dQ = weighted(view, K, ds), dK = weighted(other view, Q, ds)."""
    _, _, alpha = edge_attention_f32(src, dst, n, Q, K, V, scale, transposed)
    dV = em.weighted_f32(src, dst, n, dY, alpha, not transposed)
    dalpha = em.sddmm_f32(src, dst, n, dY, V, transposed)
    dl = edge_softmax_grad_f32(src, dst, n, alpha, dalpha, transposed)
    ds = (dl * F32(scale)).astype(F32)
    dQ = em.weighted_f32(src, dst, n, K, ds, transposed)
    dK = em.weighted_f32(src, dst, n, Q, ds, not transposed)
    return dQ, dK, dV
