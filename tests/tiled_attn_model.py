"""Exact NumPy model of the attention tiled products (include/qgtc.h, "Attention tiled products"; QGTC.tiledMMFloat(attn=) and
QGTC.tiledAggregate(attn=) on adj and adj.T): the softmax-weighted sum over each row's neighbours in ASCENDING id order, its statistics
and its three gradients, on tests/tiled_float_model.py's neighbour lists and tests/tiled_max_model.py's maximum. Every operation is
one np.float32 operation in the order the header fixes - EXP and DOT included -, so the results are compared with the device's bit for
bit. No GPU."""
import numpy as np

from tiled_float_model import neighbour_lists
from tiled_max_model import MAX, extremum_f32

F32 = np.float32

# (lanes per output row, columns per lane) of the product launchers by output width N, forward and backward mode alike: the float
# product's variants on the row view (tiled_attn_kernels.hip.h, tiled_att_f32_launch) and on the column view
# (tiled_attn_t_kernels.hip.h, tiled_att_f32_launch), both through the switches of tiled_float_kernels.hip.h. A hand-kept copy of those
# switches, as tiled_float_model.py's are. The score gradient has two variants on either view (tiled_att_grad_launch in the same two
# headers): the out node's row in registers up to N = 256, read again per neighbour beyond.
ATT_FORWARD_VARIANTS = ((16, 1), (16, 2), (16, 4), (32, 4), (64, 4))
ATT_TRANSPOSED_VARIANTS = ((16, 1), (16, 2), (16, 4))
ATT_GRAD_VARIANTS = ("registers", "reread")


def att_variant(N, transposed):
    """The template variant the product launcher picks at output width N."""
    if transposed:
        return ATT_TRANSPOSED_VARIANTS[0 if N <= 16 else 1 if N <= 32 else 2]
    return ATT_FORWARD_VARIANTS[0 if N <= 16 else 1 if N <= 32 else 2 if N <= 64 else 3 if N <= 128 else 4]


def att_chunks(N, transposed):
    """Workgroups along the output width (grid.y)."""
    lpr, cpl = att_variant(N, transposed)
    return (N + lpr * cpl - 1) // (lpr * cpl)


def att_grad_variant(N):
    return ATT_GRAD_VARIANTS[0 if N <= 256 else 1]


LOG2E, C1, C2 = F32(1.44269504088896341), F32(0.693359375), F32(-2.12194440e-4)
POLY = tuple(F32(c) for c in (1.9875691500e-4, 1.3981999507e-3, 8.3334519073e-3, 4.1665795894e-2, 1.6666665459e-1, 5.0000001201e-1))


def exp_f32(z):
    """EXP of the header for z <= 0, elementwise: 0 below -87, otherwise the Cephes expf sequence with every operation rounded to
    float32 on its own and ldexp at the end (exact: the result is a normal number)."""
    z = np.asarray(z, dtype=F32)
    small = z < F32(-87)
    with np.errstate(all="ignore"):
        zz = np.where(small, F32(0), z)            # where the result is 0 the arithmetic is not looked at
        k = np.rint(zz * LOG2E)
        r = (zz - k * C1) - k * C2
        y = np.full(z.shape, POLY[0], dtype=F32)
        for c in POLY[1:]:
            y = y * r + c
        y = (y * (r * r) + r) + F32(1)
        w = np.ldexp(y, np.nan_to_num(k, nan=0.0, posinf=0.0, neginf=0.0).astype(np.int32))
    w = np.where(small, F32(0), w)
    assert w.dtype == F32
    return w


def lrelu_f32(e, slope):
    """L(e) = e if e > 0 else fl(slope * e)."""
    e = np.asarray(e, dtype=F32)
    with np.errstate(invalid="ignore"):
        return np.where(e > 0, e, F32(slope) * e).astype(F32)


def dot_f32(x, y, fma=False):
    """DOT of the header for every row pair of x, y [R, N]: 64 in-order partial sums over the columns j, j + 64, ..., then the six
    exchange steps; float32 [R]. `fma` rounds product and add once (a WRONG rule, a test aid)."""
    x, y = np.ascontiguousarray(x, dtype=F32), np.ascontiguousarray(y, dtype=F32)
    assert x.ndim == 2 and x.shape == y.shape
    R, N = x.shape
    t = np.zeros((R, 64), dtype=F32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for c in range(0, N, 64):
            w = min(64, N - c)
            if fma:
                t[:, :w] = (t[:, :w].astype(np.float64) + x[:, c:c + w].astype(np.float64) * y[:, c:c + w].astype(np.float64)).astype(F32)
            else:
                t[:, :w] = t[:, :w] + x[:, c:c + w] * y[:, c:c + w]
        lane = np.arange(64)
        for h in (32, 16, 8, 4, 2, 1):
            t = t + t[:, lane ^ h]
    assert t.dtype == F32 and (t.view(np.uint32) == t[:, :1].view(np.uint32)).all()
    return t[:, 0].copy()


def _fold(n, group, values, descending=False):
    """out[g] = the in-order float32 sum, from +0, of values[i] over the entries i with group[i] == g; entries of one group are
    adjacent and in fold order. values is [E] or [E, N]."""
    deg = np.bincount(group, minlength=n)
    start = np.concatenate([[0], np.cumsum(deg)[:-1]])
    out = np.zeros((n,) + values.shape[1:], dtype=F32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for k in range(int(deg.max()) if deg.size and values.shape[0] else 0):
            rows = np.flatnonzero(deg > k)
            pos = start[rows] + (deg[rows] - 1 - k if descending else k)
            out[rows] = out[rows] + values[pos]
    assert out.dtype == F32
    return out


def attention_f32(src, dst, n, X, att_out, att_nbr, slope=0.2, transposed=False, wrong=None):
    """(out float32 [n, N], m float32 [n], inv float32 [n]) of the forward. `wrong` names a WRONG rule, a test aid that shows the
    inputs tell it from the contract: "descending" folds from the highest id down, "fma" rounds w * x + s once, "normalise_terms"
    multiplies every weight by inv before its term is added instead of the finished sum."""
    X = np.ascontiguousarray(X, dtype=F32)
    p, q = np.ascontiguousarray(att_out, dtype=F32), np.ascontiguousarray(att_nbr, dtype=F32)
    assert X.ndim == 2 and X.shape[0] == n and p.shape == (n,) and q.shape == (n,)
    assert wrong in (None, "descending", "fma", "normalise_terms")
    out_row, nb, deg = neighbour_lists(src, dst, n, transposed)
    if wrong == "descending":
        order = np.lexsort((-nb, out_row))
        out_row, nb = out_row[order], nb[order]
    with np.errstate(all="ignore"):
        M = extremum_f32(src, dst, n, q[:, None], transposed, MAX)[0][:, 0]
        m = lrelu_f32(p + M, slope)
        e = p[out_row] + q[nb]
        z = lrelu_f32(e, slope) - m[out_row]
        assert (z[np.isfinite(e)] <= 0).all(), "L and the rounded add are monotone: no logit exceeds the shift"
        w = exp_f32(z)
        den = _fold(n, out_row, w)
        inv = np.where(deg > 0, F32(1) / den, F32(0)).astype(F32)
        if wrong == "fma":
            start = np.concatenate([[0], np.cumsum(deg)[:-1]])
            s = np.zeros(X.shape, dtype=F32)
            for k in range(int(deg.max()) if deg.size else 0):
                rows = np.flatnonzero(deg > k)
                pos = start[rows] + k
                s[rows] = (s[rows].astype(np.float64) + w[pos, None].astype(np.float64) * X[nb[pos]].astype(np.float64)).astype(F32)
            out = s * inv[:, None]
        elif wrong == "normalise_terms":
            out = _fold(n, out_row, (w * inv[out_row])[:, None] * X[nb])
        else:
            out = _fold(n, out_row, w[:, None] * X[nb]) * inv[:, None]
    assert out.dtype == F32 and m.dtype == F32 and inv.dtype == F32
    return out, m, inv


def attention_grads_f32(src, dst, n, X, att_out, att_nbr, dY, Y, m, inv, slope=0.2, transposed=False, wrong=None):
    """(dX float32 [n, N], dp float32 [n], dq float32 [n], D float32 [n]) of the backward of attention_f32 on the same view, from its Y,
    m and inv. `wrong`: "descending" folds all three from the highest id down, "zero_is_positive" leaves the slope off an edge whose
    e is exactly 0 (the contract applies it to every e that is not > 0)."""
    X, dY, Y = (np.ascontiguousarray(t, dtype=F32) for t in (X, dY, Y))
    p, q = np.ascontiguousarray(att_out, dtype=F32), np.ascontiguousarray(att_nbr, dtype=F32)
    assert wrong in (None, "descending", "zero_is_positive")
    desc = wrong == "descending"
    o, k, _ = neighbour_lists(src, dst, n, transposed)          # the edges (out node, neighbour) sorted by (o, k)
    with np.errstate(all="ignore"):
        D = dot_f32(dY, Y)
        e = p[o] + q[k]
        w = exp_f32(lrelu_f32(e, slope) - m[o])
        alpha = w * inv[o]
        u = alpha * (dot_f32(dY[o], X[k]) - D[o]) if o.size else np.zeros(0, dtype=F32)
        plain = (e >= 0) if wrong == "zero_is_positive" else (e > 0)
        u = np.where(plain, u, F32(slope) * u).astype(F32)
        dp = _fold(n, o, u, desc)
        other = np.lexsort((o, k))                              # the other view: by (k, o)
        dq = _fold(n, k[other], u[other], desc)
        dX = _fold(n, k[other], alpha[other, None] * dY[o[other]], desc)
    assert dX.dtype == F32 and dp.dtype == F32 and dq.dtype == F32 and D.dtype == F32
    return dX, dp, dq, D
