"""The definition of uniform affine quantisation, x ~ scale * (q - zero_point), on the bit-GEMM engine (include/qgtc_affine.h,
qgtc_ppopp22_amd/affine.py), bit for bit, in NumPy. Shared by the CPU tests of the model and the GPU tests. No GPU.

All arithmetic is float32, one rounding per operation written, unless stated. qmax = 2^bits - 1, bits 1 .. 8. A group is the whole tensor
(G = 1) or one column of an [H, W] matrix (G = W).

The half-step bound. For a finite x of a group with lo <= x <= hi and scale s (not raised to its floor, not overflowed):
y = fl(x * fl(1 / s)) differs from x / s by at most |x / s| (2 u + u^2) with u = 2^-24, and |x / s| <= (hi - lo) / s <= qmax (1 + u), so by
less than 2.01 qmax u; rint adds at most 1/2; rint(y) + zero_point is an exact sum of small integers; the zero point lies within
1/2 + 2.01 qmax u of -lo / s, so the unclamped value x / s + zero_point lies within that distance of [0, qmax] and the clamp never moves the
code away from it by more. Hence |x - s (q - z)| <= s (1/2 + 3 qmax u) <= s (1/2 + 2^-14) for qmax <= 255: :data:`HALF_STEP`.

The error bounds. With element errors |ea| <= HALF_STEP sa and |eb| <= HALF_STEP sb[n],
(X + ea)(W + eb) - X W = ea W + X eb + ea eb gives
  |linear - X W|[m][n] <= (sa / 2) sum_k |W[k][n]| + (sb[n] / 2) sum_k |X[m][k]| + K sa sb[n] / 4,
times (1 + 2^-13)^2 for the slack of HALF_STEP, plus the roundings of the epilogue: fl(sa sb) and fl(t * .) are two relative errors of u on
the result, a row_scale one more, a bias one more on the sum: :func:`linear_bound` adds 4 u |result|. In the aggregate the left operand is
exact, so |aggregate - A T|[i][.] <= deg_i s / 2 with the same slack and roundings: :func:`aggregate_bound`."""
import numpy as np

TINY = np.float32(2.0 ** -100)
HALF_STEP = 0.5 + 2.0 ** -14
U = 2.0 ** -24
IDENTITY = np.array([[1.0, 0.0, 1.0, 0.0]], dtype=np.float32)    # the qparams of an operand that is its own code (the adjacency)


def _f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


def qparams(x, bits, per_column=False):
    """float32 [G, 4]: (scale, zero_point, inv_scale, 0) per group."""
    assert 1 <= bits <= 8
    x = _f32(x)
    x = x.reshape(x.shape[0], -1) if per_column else x.reshape(-1, 1)
    qmax = np.float32(2 ** bits - 1)
    fin = np.isfinite(x)
    zero = np.float32(0)
    lo = np.where(fin & (x < 0), x, zero).min(axis=0)        # +0 where nothing is below zero: a -0 element is not
    hi = np.where(fin & (x > 0), x, zero).max(axis=0)
    with np.errstate(over="ignore", divide="ignore"):
        scale = ((hi - lo).astype(np.float32) / qmax).astype(np.float32)
        scale = np.where(scale < TINY, np.where(hi == lo, np.float32(1), TINY), scale).astype(np.float32)
        inv = (np.float32(1) / scale).astype(np.float32)
        raw = np.rint(((-lo).astype(np.float32) * inv).astype(np.float32))
    zp = np.minimum(np.where(raw > 0, raw, zero), qmax).astype(np.float32)
    out = np.stack([scale, zp, inv, np.zeros_like(scale)], axis=1).astype(np.float32)
    assert out.dtype == np.float32 and out.shape == (x.shape[1], 4)
    return out


def quantise(x, qp, bits):
    """int32 codes of x [H, W] under qp [1, 4] or [W, 4]: min(max(rint(fl(x * inv_scale)) + zero_point, 0), qmax); a NaN product gives the
    zero point."""
    x, qp = _f32(x), _f32(qp)
    assert x.ndim == 2 and qp.shape in ((1, 4), (x.shape[1], 4))
    qmax = np.float32(2 ** bits - 1)
    zp, inv = qp[:, 1][None, :], qp[:, 2][None, :]
    with np.errstate(over="ignore", invalid="ignore"):
        y = (x * inv).astype(np.float32)
        r = (np.rint(y) + zp).astype(np.float32)
        c = np.minimum(np.maximum(r, np.float32(0)), qmax)
    q = np.where(np.isnan(y), np.broadcast_to(zp, y.shape), c)
    return q.astype(np.int32)


def tie_inputs(bits):
    """float32 [1, k]: the range [-2 z, 2 (qmax - z)] with z = qmax // 2, whose scale is exactly 2 and inv_scale 0.5, and every odd integer
    inside it: each x * inv_scale lies exactly on .5 and must round to even."""
    qmax = 2 ** bits - 1
    z = qmax // 2
    return np.array([[-2.0 * z, 2.0 * (qmax - z)] + [float(v) for v in range(-2 * z + 1, 2 * (qmax - z), 2)]], dtype=np.float32)


def sums(q, col_major):
    """int32: the row sums [H] of the codes in the rows layout, the column sums [W] in the cols layout."""
    return np.asarray(q, dtype=np.int64).sum(axis=0 if col_major else 1).astype(np.int32)


def dequant_t(acc, K, qa, row_sums, qb, col_sums):
    """The exact integer t [M, N] (int64) of :func:`dequant`."""
    acc, qa, qb = _f32(acc), _f32(qa), _f32(qb)
    M, N = acc.shape
    assert qa.shape == (1, 4) and qb.shape in ((1, 4), (N, 4))
    za = int(qa[0, 1])
    zb = np.broadcast_to(qb[:, 1].astype(np.int64), (N,))
    t = acc.astype(np.int64) + int(K) * za * zb[None, :]
    if row_sums is not None:
        t = t - zb[None, :] * np.asarray(row_sums, dtype=np.int64)[:, None]
    if col_sums is not None:
        t = t - za * np.asarray(col_sums, dtype=np.int64)[None, :]
    return t


def dequant(acc, K, qa, row_sums, qb, col_sums, row_scale=None, bias=None, relu=False):
    """float32 [M, N]: fl(float(t) * fl(sa * sb[n])), then * row_scale[m], + bias[n], and out > 0 ? out : +0 under relu."""
    qa, qb = _f32(qa), _f32(qb)
    t = dequant_t(acc, K, qa, row_sums, qb, col_sums)
    N = t.shape[1]
    s = (qa[0, 0] * np.broadcast_to(qb[:, 0], (N,))).astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        out = (t.astype(np.float32) * s[None, :]).astype(np.float32)         # int64 -> float32 rounds to nearest even
        if row_scale is not None:
            out = (out * _f32(row_scale)[:, None]).astype(np.float32)
        if bias is not None:
            out = (out + _f32(bias)[None, :]).astype(np.float32)
    if relu:
        out = np.where(out > 0, out, np.float32(0)).astype(np.float32)
    assert out.dtype == np.float32
    return out


def linear_parts(X, W, a_bits, w_bits, per_column=True):
    """(qa, codes of X, qb, codes of W, acc float32 [M, N]) of :func:`linear`."""
    X, W = _f32(X), _f32(W)
    qa, qb = qparams(X, a_bits), qparams(W, w_bits, per_column)
    cx, cw = quantise(X, qa, a_bits), quantise(W, qb, w_bits)
    acc = (cx.astype(np.int64) @ cw.astype(np.int64))
    assert int(acc.max(initial=0)) < 2 ** 24, "the accumulator must be exact in float32"
    return qa, cx, qb, cw, acc.astype(np.float32)


def linear(X, W, a_bits, w_bits, per_column=True, row_scale=None, bias=None, relu=False):
    qa, cx, qb, cw, acc = linear_parts(X, W, a_bits, w_bits, per_column)
    return dequant(acc, X.shape[1], qa, sums(cx, False), qb, sums(cw, True), row_scale, bias, relu)


def dense_view(src, dst, n, transposed=False):
    """int64 [n, n]: the 1-bit adjacency of the edge list as the view's matrix (multiplicities 1, 2, >= 3 quantise to 1, 0, 1)."""
    from tiled_model import set_cells

    cells = set_cells(src, dst, n)
    A = np.zeros((n, n), dtype=np.int64)
    A[cells // n, cells % n] = 1
    return A.T.copy() if transposed else A


def masked_view(A, row_mask=None, nbr_mask=None):
    A = np.asarray(A, dtype=np.int64)
    if row_mask is not None:
        A = A * np.asarray(row_mask, dtype=np.int64)[:, None]
    if nbr_mask is not None:
        A = A * np.asarray(nbr_mask, dtype=np.int64)[None, :]
    return A


def aggregate(A, T, bits, row_scale=None, row_mask=None, nbr_mask=None):
    """float32 [n, N]: the neighbour sum of T on the view's matrix A (int [n, n] of 0 / 1; the masks are bool [n] or None), T quantised
    per tensor: dequant(exact sum of the codes, n, IDENTITY, the degrees under the masks, qT, None, row_scale)."""
    T = _f32(T)
    Am = masked_view(A, row_mask, nbr_mask)
    qt = qparams(T, bits)
    acc = Am @ quantise(T, qt, bits).astype(np.int64)
    assert int(acc.max(initial=0)) < 2 ** 24
    return dequant(acc.astype(np.float32), A.shape[0], IDENTITY, Am.sum(axis=1), qt, None, row_scale)


def inv_degree(deg):
    deg = np.asarray(deg)
    with np.errstate(divide="ignore"):
        inv = np.float32(1) / deg.astype(np.float32)
    return np.where(deg == 0, np.float32(0), inv).astype(np.float32)


def inv_sqrt_degree(deg):
    d = np.asarray(deg).astype(np.float32)
    out = np.zeros(d.shape, dtype=np.float32)
    out[d > 0] = np.float32(1) / np.sqrt(d[d > 0])
    return out


def norm_scales(A, norm, nodes=None):
    """(row, src) float32 [n] or None of the layer's norm on the view's matrix A under the node set."""
    Am = masked_view(A, nodes, nodes)
    if norm == "mean":
        return inv_degree(Am.sum(axis=1)), None
    if norm == "sym":
        return inv_sqrt_degree(Am.sum(axis=1)), inv_sqrt_degree(Am.sum(axis=0))
    assert norm is None
    return None, None


def gcn(A, X, W_in, W_out, w_bit, act_bit, norm=None, nodes=None):
    """affine.GCNConv_Affine.forward on the view's matrix A: agg(linear(agg(linear(X, W_in)), W_out)), weights per output column."""
    row, src = norm_scales(A, norm, nodes)
    h = aggregate(A, linear(X, W_in, act_bit, w_bit, True, row_scale=src), act_bit, row, nodes, nodes)
    return aggregate(A, linear(h, W_out, act_bit, w_bit, True, row_scale=src), act_bit, row, nodes, nodes)


def gcn_f64(A, X, W_in, W_out, norm=None, nodes=None):
    """The float64 layer pair the quantised one approximates."""
    row, src = norm_scales(A, norm, nodes)
    Am = masked_view(A, nodes, nodes).astype(np.float64)
    if src is not None:
        Am = Am * src.astype(np.float64)[None, :]
    if row is not None:
        Am = Am * row.astype(np.float64)[:, None]
    f = lambda a: np.asarray(a, dtype=np.float64)
    return Am @ ((Am @ (f(X) @ f(W_in))) @ f(W_out))


def rel_error(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.linalg.norm(got - want) / np.linalg.norm(want))


def linear_bound(X, W, qa, qb, result):
    """float64 [M, N]: the bound of the module docstring on |linear - X W| (no row_scale, bias or relu)."""
    X, W = np.asarray(X, dtype=np.float64), np.asarray(W, dtype=np.float64)
    sa, sb = float(qa[0, 0]), np.broadcast_to(np.asarray(qb, dtype=np.float64)[:, 0], (W.shape[1],))
    first = sa / 2 * np.abs(W).sum(axis=0)[None, :] + sb[None, :] / 2 * np.abs(X).sum(axis=1)[:, None] + X.shape[1] * sa * sb[None, :] / 4
    return first * (1 + 2.0 ** -13) ** 2 + 4 * U * np.abs(np.asarray(result, dtype=np.float64))


def aggregate_bound(A, qt, result, row_scale=None):
    """float64 [n, 1]-broadcastable: the bound on |aggregate - r A T|."""
    deg = np.asarray(A, dtype=np.float64).sum(axis=1)
    r = np.ones_like(deg) if row_scale is None else np.asarray(row_scale, dtype=np.float64)
    return (r * deg * float(qt[0, 0]) / 2 * (1 + 2.0 ** -13))[:, None] + 4 * U * np.abs(np.asarray(result, dtype=np.float64))
