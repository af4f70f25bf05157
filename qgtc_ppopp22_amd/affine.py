"""Uniform affine quantisation on the bit-GEMM engine (include/qgtc_affine.h): x ~ scale * (q - zero_point), with
the range taken from the data on the device, so that real-valued features and trained weights run through ``bitMM2Int`` / ``tiledMM2Int``
and come back in real units. tests/affine_model.py states every bit of it in NumPy.

    qp = affine.qparams(x, bits)                          # float32 [G, 4]: (scale, zero_point, inv_scale, 0) per group, on the device
    words, sums = affine.val2bit_affine(x, bits, qp)      # the layouts of QGTC.val2bit(x, bits, col_major, False), and the code sums
    y = affine.dequant(acc, K, qa, row_sums, qb, col_sums)
    y = affine.linear(X, W, 8, 4)                         # ~ X @ W
    y = affine.linear(X, W, 8, 4, route="bytes")          # the same bits from one int8 MFMA launch on byte codes (include/qgtc_linear.h)
    wt, qw, sums = affine.pack_weight(W, 4)               # W's codes transposed (uint8 [N, PAD16(K)]), its qparams rows and column sums
    y = affine.aggregate(adj, T, 8)                       # ~ A . T on a QGTC.TiledAdjacency view
    y = affine.aggregate(adj, T, 8, route="bytes")        # the same bits from one walk over byte codes (include/qgtc_codes.h)
    q = affine.codes(x, bits, qp)                         # uint8 [H, W], one byte a code, rows PAD4(W) bytes apart
    acc = affine.tiledMMCodes(adj, q)                     # int32 [n, N]: the exact neighbour sum of the codes
    layer = affine.GCNConv_Affine.from_float(trained_gcnconv, 4, 8)
    q = affine.linear(X, W, 8, 4, route="bytes", x_qparams=qx, out=(8, qy))   # static: fixed rows, uint8 codes out (or in: uint8 X)
    q = affine.aggregate(adj, q, 8, route="bytes", t_qparams=qy, out=(8, qz)) # codes in, codes out: include/qgtc_chain.h
    rows = layer.calibrate(A, X);  y = layer(A, X, act_qparams=rows)          # the layer as a chain of six launches
    q = affine.aggregate_linear(adj, q, qy, (8, qz), W, 4, out=(8, qo))       # the middle walk and the product behind it, one launch
    y = layer(A, X, act_qparams=rows, fuse=True)                              # five launches, the same bits: include/qgtc_fused.h
    y = affine.aggregate(adj, T, 8, route="bytes", edge_weight=alpha)         # ~ sum_k alpha[slot] T[k]: include/qgtc_codes_edge.h
    layer = affine.TransformerConv_Affine.from_float(trained_transformerconv, 4, 8)   # likewise GATv2Conv_Affine
    m = affine.tiledMaxCodes(adj, q, reduce="max")        # uint8 [n, N]: the extremum of the neighbours' codes, itself a code under q's row
    y = affine.aggregate(adj, T, 8, route="bytes", reduce="max")              # ~ max over the neighbours' rows of T: include/qgtc_codes_max.h
    layer = affine.GCNConv_Affine.from_float(gcnconv_with_aggr_max, 4, 8, route="bytes", linear_route="bytes")

The C entries (four of include/qgtc_affine.h, five of include/qgtc_codes.h, two of include/qgtc_linear.h, three of include/qgtc_chain.h, one of include/qgtc_fused.h, four of include/qgtc_codes_max.h, two of include/qgtc_codes_edge.h) are reached through ctypes on torch's current stream (the
extension binds no name for them): every call enqueues, reads nothing back and can be captured into a graph; the quantisation parameters stay on the device, so a replay follows the data's
range. The outputs and the scratch of the range launch are allocated here. Inference only: nothing here is differentiable, and no output
requires grad. The accumulators of the planes route are float32 holding integers: there ``linear`` refuses a K at which
K * qmax_a * qmax_w could pass 2^24; its bytes route accumulates in int32 and refuses K above ``LINEAR_K_MAX`` only."""
from __future__ import annotations

import math

import torch

import QGTC  # the HIP extension; there is no fallback

from . import conv, tiled
from .tiled import _c_abi, _ptr

__all__ = ["qparams", "val2bit_affine", "dequant", "linear", "aggregate", "GCNConv_Affine", "codes", "tiledMMCodes", "pack_weight", "aggregate_linear", "tiledMaxCodes",
           "TransformerConv_Affine", "GATv2Conv_Affine"]

ROUTES = ("planes", "bytes")   # how ``aggregate`` sums the codes: eight bit planes through tiledMM2Int, or one gather of byte codes
REDUCES = ("sum", "max", "min")   # the reducer of ``aggregate`` and of the layer's ``aggr``; an extremum is served on route="bytes" only
FUSED_MAX = 256                # QGTC_FUSED_K_MAX and QGTC_FUSED_N_MAX of include/qgtc_fused.h: the widths one workgroup holds
LINEAR_K_MAX = 131071          # QGTC_LINEAR_K_MAX of include/qgtc_linear.h: K 2^14 < 2^31, the int32 accumulator of the shifted codes

_identity = {}   # per device: the qparams row (1, 0, 1, 0) of an operand that is its own code; a constant, built outside captures


def _c_call(what: str, on: torch.Tensor, fn, *args) -> None:
    """``tiled._c_call``, with the runtime's own words added to a HIP error."""
    try:
        tiled._c_call(what, on, fn, *args)
    except RuntimeError as e:
        text = _c_abi().qgtc_last_hip_error().decode()
        raise RuntimeError(f"{e}: {text}" if text else str(e)) from None


def _check_bits(bits, name="bits") -> int:
    if isinstance(bits, bool) or not isinstance(bits, int):
        raise TypeError(f"{name} must be an int in 1 .. 8, not {bits!r}")
    if not 1 <= bits <= 8:
        raise ValueError(f"{name} must lie in 1 .. 8, not {bits}")
    return bits


def _check_f32(t, name: str, dims: int | None = 2) -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, not {type(t).__name__}")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, not {t.dtype}")
    if not t.is_cuda:
        raise ValueError(f"{name} must be on a GPU, not on {t.device}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if dims is not None and t.dim() != dims:
        raise ValueError(f"{name} must have {dims} dimensions, not shape {list(t.shape)}")
    if t.numel() == 0:
        raise ValueError(f"{name} must not be empty (shape {list(t.shape)})")


def _check_qparams(qp, name: str, allowed: tuple, like: torch.Tensor) -> int:
    _check_f32(qp, name)
    if qp.size(1) != 4 or qp.size(0) not in allowed:
        raise ValueError(f"{name} must have shape [G, 4] with G in {sorted(set(allowed))} (affine.qparams), not {list(qp.shape)}")
    if qp.device != like.device:
        raise ValueError(f"{name} must be on {like.device}, not on {qp.device}")
    return int(qp.size(0))


def _check_vector(t, name: str, dtype, n: int, like: torch.Tensor) -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor or None, not {type(t).__name__}")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, not {t.dtype}")
    if t.dim() != 1 or t.numel() != n:
        raise ValueError(f"{name} must have shape [{n}], not {list(t.shape)}")
    if t.device != like.device:
        raise ValueError(f"{name} must be on {like.device}, not on {t.device}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def qparams(x: torch.Tensor, bits: int, per_column: bool = False) -> torch.Tensor:
    """float32 [G, 4] on x's device: (scale, zero_point, inv_scale, 0) of the whole tensor (G = 1) or of every column of x [H, W]
    (``per_column``, G = W), from the finite elements' range extended to 0. Two launches (partials, then the finish); no host read."""
    bits = _check_bits(bits)
    _check_f32(x, "x")
    H, W = x.shape
    L = _c_abi()
    out = torch.empty((W if per_column else 1, 4), dtype=torch.float32, device=x.device)
    work = torch.empty((max(1, L.qgtc_affine_work_words(H, W, int(bool(per_column)))),), dtype=torch.int32, device=x.device)
    _c_call("affine.qparams", x, L.qgtc_affine_qparams, x.data_ptr(), H, W, bits, int(bool(per_column)), out.data_ptr(), out.numel(),
            work.data_ptr(), work.numel())
    return out


def val2bit_affine(x: torch.Tensor, bits: int, qp: torch.Tensor, col_major: bool = False, return_sums: bool = True):
    """(words, sums): x [H, W] quantised with ``qp`` ([1, 4]: per tensor; [W, 4]: per column) and packed as
    ``QGTC.val2bit(codes, bits, col_major, False)`` packs - int32 [bits * PAD8(H), S128(W) * 4] in the rows layout,
    [bits * S128(H) * 4, PAD128(W)] in the cols layout, every pad word written. ``sums`` is int32 [H] (row sums of the codes) in the
    rows layout and [W] (column sums) in the cols layout, or None without ``return_sums``."""
    bits = _check_bits(bits)
    _check_f32(x, "x")
    H, W = x.shape
    groups = _check_qparams(qp, "qp", (1, W), x)
    if col_major:
        out = torch.empty((bits * ((H + 127) // 128) * 4, (W + 127) // 128 * 128), dtype=torch.int32, device=x.device)
    else:
        out = torch.empty((bits * ((H + 7) // 8 * 8), (W + 127) // 128 * 4), dtype=torch.int32, device=x.device)
    sums = torch.empty((W if col_major else H,), dtype=torch.int32, device=x.device) if return_sums else None
    _c_call("affine.val2bit_affine", x, _c_abi().qgtc_val2bit_affine, x.data_ptr(), H, W, bits, int(bool(col_major)), qp.data_ptr(), groups,
            out.data_ptr(), out.numel(), _ptr(sums), 0 if sums is None else sums.numel())
    return out, sums


def dequant(acc: torch.Tensor, K: int, qa: torch.Tensor, row_sums, qb: torch.Tensor, col_sums, row_scale=None, bias=None,
            relu: bool = False, out: torch.Tensor | None = None) -> torch.Tensor:
    """float32 [M, N] = (acc - zb row_sums - za col_sums + K za zb) * (sa * sb), the integer part exact in 64 bits, then ``* row_scale[m]``,
    ``+ bias[n]`` and a relu when given. ``acc`` is the product of the codes over K terms (``bitMM2Int`` / ``tiledMM2Int``), ``qa`` [1, 4]
    the left operand's parameters, ``qb`` [1, 4] or [N, 4] the right operand's, ``row_sums`` int32 [M] / ``col_sums`` int32 [N] the code
    sums (None: the term is left out - the caller asserts the other zero point is 0). ``out`` may be ``acc`` (in place)."""
    _check_f32(acc, "acc")
    M, N = acc.shape
    if isinstance(K, bool) or not isinstance(K, int):
        raise TypeError(f"K must be an int, not {K!r}")
    if not 1 <= K < 2 ** 31:
        raise ValueError(f"K must lie in 1 .. 2^31 - 1, not {K}")
    _check_qparams(qa, "qa", (1,), acc)
    groups_b = _check_qparams(qb, "qb", (1, N), acc)
    for t, name, dtype, n in ((row_sums, "row_sums", torch.int32, M), (col_sums, "col_sums", torch.int32, N),
                              (row_scale, "row_scale", torch.float32, M), (bias, "bias", torch.float32, N)):
        if t is not None:
            _check_vector(t, name, dtype, n, acc)
    if out is None:
        out = torch.empty_like(acc)
    else:
        _check_f32(out, "out")
        if out.shape != acc.shape or out.device != acc.device:
            raise ValueError(f"out must have shape {list(acc.shape)} on {acc.device}, not {list(out.shape)} on {out.device}")
    _c_call("affine.dequant", acc, _c_abi().qgtc_affine_dequant, acc.data_ptr(), M, N, K, qa.data_ptr(), _ptr(row_sums), qb.data_ptr(),
            groups_b, _ptr(col_sums), _ptr(row_scale), _ptr(bias), int(bool(relu)), out.data_ptr(), out.numel())
    return out


def pack_weight(W: torch.Tensor, bits: int, per_column: bool = True):
    """(codes_t, qparams, col_sums) of W [K, N] for ``linear(route="bytes")``, from one launch: ``qparams`` float32 [N, 4] (per output
    column) or [1, 4] (per tensor), bit for bit ``affine.qparams(W, bits, per_column)``; ``codes_t`` uint8 [N, PAD16(K)], W's codes
    transposed so that a column's K codes are contiguous, bytes K .. PAD16(K) - 1 of every line written 0; ``col_sums`` int32 [N]."""
    bits = _check_bits(bits)
    _check_f32(W, "W")
    K, N = W.shape
    if K > LINEAR_K_MAX:
        raise ValueError(f"K = {K}: the int32 accumulator of the bytes route holds K up to {LINEAR_K_MAX}")
    ldk = (K + 15) // 16 * 16
    qp = torch.empty((N if per_column else 1, 4), dtype=torch.float32, device=W.device)
    codes_t = torch.empty((N, ldk), dtype=torch.uint8, device=W.device)
    col_sums = torch.empty((N,), dtype=torch.int32, device=W.device)
    _c_call("affine.pack_weight", W, _c_abi().qgtc_affine_pack_weight, W.data_ptr(), K, N, bits, int(bool(per_column)), qp.data_ptr(),
            qp.numel(), codes_t.data_ptr(), ldk, codes_t.numel(), col_sums.data_ptr(), col_sums.numel())
    return codes_t, qp, col_sums


def linear(X: torch.Tensor, W: torch.Tensor, a_bits: int, w_bits: int, per_column: bool = True, row_scale=None, bias=None,
           relu: bool = False, route: str = "planes", x_qparams=None, out=None) -> torch.Tensor:
    """float32 [M, N] ~ X @ W on the bit-GEMM: X [M, K] quantised per tensor to ``a_bits`` (rows layout), W [K, N] per output column (or
    per tensor) to ``w_bits`` (cols layout, as ``GCNConv_Qnt.weight_Qnt`` packs weights), ``QGTC.bitMM2Int`` on the codes, then
    :func:`dequant` with the row sums of X's codes and the column sums of W's. Element [m][n] is within
    (sa / 2) sum_k |W[k][n]| + (sb[n] / 2) sum_k |X[m][k]| + K sa sb[n] / 4 of the exact product (to first order).

    ``route="bytes"`` gives the same bits from byte codes on the int8 matrix instruction (include/qgtc_linear.h):
    :func:`qparams` of X, :func:`pack_weight` of W, then one launch that reads X, quantises it in registers, multiplies into an int32
    accumulator and dequantises - four launches, no packed X, no intermediate. Exact for every K up to ``LINEAR_K_MAX``; the 2^24 limit
    below belongs to the planes route.

    Static quantisation, on the bytes route only (include/qgtc_chain.h). ``x_qparams`` (float32 [1, 4]) fixes
    X's row: no range launches are made. X may then be uint8 [M, K] (unit column stride), codes under that row, taken as they are.
    ``out=(bits, row)`` returns the result's codes under the fixed per-tensor ``row`` instead of float32: uint8 [M, N], a view of a
    buffer with rows PAD16(N) bytes apart - bit for bit ``codes(linear(...), bits, row)``, from the product's own epilogue."""
    route = _check_route(route)
    a_bits, w_bits = _check_bits(a_bits, "a_bits"), _check_bits(w_bits, "w_bits")
    coded = isinstance(X, torch.Tensor) and X.dtype == torch.uint8
    if route != "bytes" and (coded or x_qparams is not None or out is not None):
        raise ValueError('uint8 X, x_qparams= and out= need route="bytes"')
    if coded:
        X = _check_u8(X, "X")
        if x_qparams is None:
            raise ValueError("uint8 X needs x_qparams, the row its codes were made under")
    else:
        _check_f32(X, "X")
    _check_f32(W, "W")
    M, K = X.shape
    if W.size(0) != K or W.device != X.device:
        raise ValueError(f"W must have shape [{K}, N] on {X.device}, not {list(W.shape)} on {W.device}")
    N = W.size(1)
    if route == "bytes":
        if K > LINEAR_K_MAX:
            raise ValueError(f"K = {K}: the int32 accumulator of the bytes route holds K up to {LINEAR_K_MAX}")
        for t, name, n in ((row_scale, "row_scale", M), (bias, "bias", N)):
            if t is not None:
                _check_vector(t, name, torch.float32, n, X)
        if x_qparams is not None:
            _check_qparams(x_qparams, "x_qparams", (1,), X)
        out_bits, out_qp = _check_out(out, X)
        qa = qparams(X, a_bits) if x_qparams is None else x_qparams
        codes_t, qb, col_sums = pack_weight(W, w_bits, per_column)
        L = _c_abi()
        right = (codes_t.data_ptr(), codes_t.size(1), codes_t.numel(), N, qb.data_ptr(), qb.size(0), col_sums.data_ptr(), _ptr(row_scale),
                 _ptr(bias), int(bool(relu)))
        if not coded and out is None:
            res = torch.empty((M, N), dtype=torch.float32, device=X.device)
            _c_call("affine.linear", X, L.qgtc_affine_linear_u8, X.data_ptr(), M, K, qa.data_ptr(), a_bits, *right, res.data_ptr(), res.numel())
            return res
        left = (None, X.data_ptr(), _codes_ld(X), _codes_bytes(X)) if coded else (X.data_ptr(), None, 0, 0)
        res, flt, mat, row = _dest(out, out_bits, out_qp, M, N, X.device)
        _c_call("affine.linear", X, L.qgtc_affine_linear_chain, *left, M, K, qa.data_ptr(), a_bits, *right, *flt, *mat, *row)
        return res
    if K * (2 ** a_bits - 1) * (2 ** w_bits - 1) >= 2 ** 24:
        raise ValueError(f"K = {K} at a_bits = {a_bits}, w_bits = {w_bits}: the float32 accumulator of bitMM2Int is exact below 2^24 only")
    qa = qparams(X, a_bits)
    bit_X, row_sums = val2bit_affine(X, a_bits, qa, False, True)
    qb = qparams(W, w_bits, per_column)
    bit_W, col_sums = val2bit_affine(W, w_bits, qb, True, True)
    acc = QGTC.bitMM2Int(bit_X, bit_W, M, K, N, a_bits, w_bits, True)   # pad_128: W's planes are PAD128(N) lines apart
    return dequant(acc, K, qa, row_sums, qb, col_sums, row_scale, bias, relu, out=acc)


def _check_out(out, like: torch.Tensor):
    """``out=(bits, row)`` of the static calls as (bits, row), the row checked as a per-tensor qparams row; (0, None) without."""
    if out is None:
        return 0, None
    if not isinstance(out, tuple) or len(out) != 2:
        raise TypeError(f"out must be a tuple (bits, qparams row), not {out!r}")
    bits = _check_bits(out[0], "out bits")
    _check_qparams(out[1], "out qparams", (1,), like)
    return bits, out[1]


def _dest(out, out_bits: int, out_qp, rows: int, cols: int, device):
    """(res, flt, mat, row): the result of a static call and its destination arguments in three named parts - ``flt`` (out, out_elems),
    ``mat`` (outq, ldo, outq_bytes) and ``row`` (out_qp, out_bits); the C entries take ``*flt, *mat, *row``, the requant walks
    ``*row, *mat``. float32 [rows, cols] without ``out=``, the code matrix of :func:`_codes_out` with."""
    if out is None:
        res = torch.empty((rows, cols), dtype=torch.float32, device=device)
        return res, (res.data_ptr(), res.numel()), (None, 0, 0), (None, 0)
    buf, res = _codes_out(rows, cols, device)
    return res, (None, 0), (buf.data_ptr(), buf.size(1), buf.numel()), (out_qp.data_ptr(), out_bits)


def _codes_out(M: int, N: int, device):
    """(buffer, view): uint8 [M, PAD16(N)] and its columns :N, the code matrix a static call writes - rows 16-byte aligned, so that the
    next product loads them 16 bytes at a time."""
    buf = torch.empty((M, (N + 15) // 16 * 16), dtype=torch.uint8, device=device)
    return buf, buf[:, :N]


def _identity_qparams(device: torch.device) -> torch.Tensor:
    """float32 [1, 4] = (1, 0, 1, 0), made by fills on the device (no host copy: capturable); kept per device when made outside a capture."""
    key = (device.type, device.index)
    t = _identity.get(key)
    if t is None:
        t = torch.zeros((1, 4), dtype=torch.float32, device=device)
        t[:, 0::2] = 1.0
        if not torch.cuda.is_current_stream_capturing():
            _identity[key] = t
    return t


def _check_reduce(reduce, name: str = "reduce") -> str:
    if reduce not in REDUCES:
        raise ValueError(f'{name} must be "sum", "max" or "min", not {reduce!r}')
    return reduce


def _check_route(route) -> str:
    if route not in ROUTES:
        raise ValueError(f'route must be "planes" or "bytes", not {route!r}')
    return route


def _pad4(W: int) -> int:
    return (W + 3) // 4 * 4


def codes(x: torch.Tensor, bits: int, qp: torch.Tensor) -> torch.Tensor:
    """uint8 [H, W]: x quantised with ``qp`` ([1, 4]: per tensor; [W, 4]: per column) by the rule of :func:`val2bit_affine`, one byte a
    code - a view of a [H, PAD4(W)] buffer (row stride PAD4(W)), whose bytes W .. PAD4(W) - 1 of every row are written 0. One launch."""
    bits = _check_bits(bits)
    _check_f32(x, "x")
    H, W = x.shape
    groups = _check_qparams(qp, "qp", (1, W), x)
    ld = _pad4(W)
    buf = torch.empty((H, ld), dtype=torch.uint8, device=x.device)
    _c_call("affine.codes", x, _c_abi().qgtc_affine_codes, x.data_ptr(), H, W, bits, qp.data_ptr(), groups, buf.data_ptr(), ld, buf.numel())
    return buf[:, :W]


def _check_codes(adj_view, Q, name: str = "Q") -> torch.Tensor:
    """Q as the C entries take it: any 2-D uint8 with unit column stride; a row stride or a base address off the 4-byte rule of a code
    matrix (include/qgtc_codes.h) gets a padded copy."""
    if isinstance(Q, torch.Tensor) and Q.dtype == torch.uint8 and Q.is_cuda and Q.dim() == 2 and Q.numel() and (
            Q.size(0) != adj_view.n or Q.device != adj_view.device):
        raise ValueError(f"{name} must have shape [{adj_view.n}, N] on {adj_view.device}, not {list(Q.shape)} on {Q.device}")
    return _check_u8(Q, name)


def _check_u8(Q, name: str) -> torch.Tensor:
    if not isinstance(Q, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, not {type(Q).__name__}")
    if Q.dtype != torch.uint8:
        raise TypeError(f"{name} must be uint8, not {Q.dtype}")
    if not Q.is_cuda:
        raise ValueError(f"{name} must be on a GPU, not on {Q.device}")
    if Q.dim() != 2:
        raise ValueError(f"{name} must have 2 dimensions, not shape {list(Q.shape)}")
    if Q.numel() == 0:
        raise ValueError(f"{name} must not be empty (shape {list(Q.shape)})")
    if Q.stride(1) != 1 and Q.size(1) > 1:
        raise ValueError(f"{name} must have unit column stride, not strides {list(Q.stride())}")
    n, N = Q.shape
    ld = _codes_ld(Q)
    if ld < N or ld % 4 or Q.data_ptr() % 4 or Q.stride(1) != 1 or _codes_bytes(Q) < (n - 1) * ld + _pad4(N):
        buf = torch.empty((n, _pad4(N)), dtype=torch.uint8, device=Q.device)   # (the pad bytes may hold anything)
        buf[:, :N] = Q
        Q = buf[:, :N]
    return Q


def _codes_ld(Q: torch.Tensor) -> int:
    """The row stride in bytes; a single row, whose stride torch leaves arbitrary, counts as PAD4(N) apart."""
    return Q.stride(0) if Q.size(0) > 1 else _pad4(Q.size(1))


def _codes_bytes(Q: torch.Tensor) -> int:
    """The bytes the storage holds from Q's first byte on."""
    return Q.untyped_storage().nbytes() - Q.storage_offset()


def _check_masks(adj_view, row_mask, nbr_mask) -> None:
    for m, name in ((row_mask, "row_mask"), (nbr_mask, "nbr_mask")):
        if m is not None:
            tiled._check_mask(adj_view, m, name)


def _codes_args(Q: torch.Tensor) -> tuple:
    """A code matrix as the C entries take it: (pointer, row stride, bytes from the first on, columns)."""
    return Q.data_ptr(), _codes_ld(Q), _codes_bytes(Q), Q.size(1)


def _u8_call(what: str, stem: str, suffix: str, adj_view, Q: torch.Tensor, row_mask, nbr_mask, *args) -> None:
    """The walk entry ``stem`` [``_t`` on the transposed view] ``suffix`` on the view's index arrays, Q, ``args`` and the masks."""
    fn = getattr(_c_abi(), stem + ("_t" if adj_view.transposed else "") + suffix)
    _c_call(what, Q, fn, *tiled._view_args(adj_view), *_codes_args(Q), *args, _ptr(row_mask), _ptr(nbr_mask), adj_view.mask_words)


def tiledMMCodes(adj_view: "tiled.TiledAdjacency", Q: torch.Tensor, row_mask=None, nbr_mask=None) -> torch.Tensor:
    """int32 [n, N]: the exact sum of the code rows Q[k] (uint8 [n, N], in the adjacency's numbering) over the neighbours k of every row
    of the view ``adj_view`` (``adj`` or ``adj.T``), under the node masks of :func:`QGTC.tiledMM2Int` - what ``tiledMM2Int`` gives on the
    packed planes of the same codes, from one walk that gathers one dword of four codes per neighbour. One launch."""
    tiled._check(adj_view)
    Q = _check_codes(adj_view, Q)
    _check_masks(adj_view, row_mask, nbr_mask)
    out = torch.empty((adj_view.n, Q.size(1)), dtype=torch.int32, device=Q.device)
    _u8_call("affine.tiledMMCodes", "qgtc_tiledmm_u8", "", adj_view, Q, row_mask, nbr_mask, out.data_ptr(), out.numel())
    return out


def tiledMaxCodes(adj_view: "tiled.TiledAdjacency", Q: torch.Tensor, reduce: str = "max", empty: int = 0, row_mask=None,
                  nbr_mask=None) -> torch.Tensor:
    """uint8 [n, N]: the element-wise maximum (``reduce="max"``) or minimum ("min") of the code rows Q[k] (uint8 [n, N], in the
    adjacency's numbering) over the neighbours k of every row of the view ``adj_view`` (``adj`` or ``adj.T``), under the node masks of
    :func:`tiledMMCodes` (include/qgtc_codes_max.h). The quantiser is monotone, so the result is the code of the
    extremum under Q's own qparams row, with no error of its own. A row without a live neighbour, or outside ``row_mask``, holds
    ``empty`` (0 .. 255). A view of a buffer with rows PAD16(N) bytes apart, bytes N .. PAD4(N) - 1 written 0. One launch."""
    tiled._check(adj_view)
    Q = _check_codes(adj_view, Q)
    if _check_reduce(reduce) == "sum":
        raise ValueError('reduce must be "max" or "min" here: tiledMMCodes is the sum')
    if isinstance(empty, bool) or not isinstance(empty, int):
        raise TypeError(f"empty must be an int in 0 .. 255, not {empty!r}")
    if not 0 <= empty <= 255:
        raise ValueError(f"empty must lie in 0 .. 255, not {empty}")
    _check_masks(adj_view, row_mask, nbr_mask)
    buf, res = _codes_out(adj_view.n, Q.size(1), Q.device)
    _u8_call("affine.tiledMaxCodes", "qgtc_tiledmax_u8", "", adj_view, Q, row_mask, nbr_mask, int(reduce == "min"), empty, buf.data_ptr(),
             buf.size(1), buf.numel())
    return res


def aggregate(adj_view: "tiled.TiledAdjacency", T: torch.Tensor, bits: int, row_scale=None, row_mask=None, nbr_mask=None,
              route: str = "planes", t_qparams=None, out=None, reduce: str = "sum", edge_weight=None) -> torch.Tensor:
    """float32 [n, N] ~ A . T on the view ``adj_view`` (``adj`` or ``adj.T``; T in the adjacency's numbering): T quantised per tensor to
    ``bits`` into the cols layout, ``QGTC.tiledMM2Int`` on the codes (the exact neighbour sum), then :func:`dequant` with the view's
    degrees under the masks as the row sums of A, and ``row_scale`` (float32 [n], say ``adj_view.mean_scale()``) applied there. Row i is
    within deg_i * scale / 2 of the exact sum; a row without live neighbours, or outside ``row_mask``, comes back +0.

    ``route="bytes"`` gives the same bits from byte codes (include/qgtc_codes.h): :func:`qparams`, :func:`codes`,
    then one launch that gathers the neighbours' codes, counts the terms of every row and dequantises in its epilogue - four launches, no
    degree launch and no integer intermediate.

    Static quantisation, on the bytes route only (include/qgtc_chain.h). ``t_qparams`` (float32 [1, 4]) fixes
    T's row: no range launches. T may then be uint8 [n, N], codes under that row: the walk is the only launch. ``out=(bits, row)``
    returns the result's codes under the fixed ``row`` (uint8 [n, N], rows PAD16(N) apart), bit for bit ``codes(aggregate(...), bits,
    row)``; a row without live neighbours, or outside ``row_mask``, is float +0 and so the row's zero point.

    ``reduce="max"`` / ``"min"``, on the bytes route only (include/qgtc_codes_max.h), replace the sum by the
    element-wise extremum over the neighbours: scale * (m - zero_point) with m the extremum of the neighbours' codes, which is the
    quantised value of the extremum itself - the aggregate adds no error to T's quantisation. Float T, uint8 T with ``t_qparams`` and
    ``out=(bits, row)`` work as for the sum; ``row_scale`` is a ValueError (an extremum is not scaled); a row without a term is +0.

    ``edge_weight`` (float32 [nnz], or [nnz, H] for H heads, in slot order: ``tiled.edge_values``, ``tiled.tiledEdgeSoftmax``), on the
    bytes route and the sum only (include/qgtc_codes_edge.h), weighs every term:
    ``scale * sum_k w[slot(o, k), c // (N / H)] * (q[k][c] - zero_point)`` - the sum every attention layer ends in, gathered one byte an
    element. Float T, uint8 T with ``t_qparams``, ``out=(bits, row)``, ``row_scale`` and both masks work as for the plain sum; a
    masked-out cell keeps its slot, so the masks only drop terms. The sum is float32 with fused multiply-adds and no fixed order: within
    (terms + 4) 2^-23 scale |row_scale| (255 + zero_point) sum|w| of the exact value. With H > 1 a head's N / H columns must be a
    multiple of 4; other shapes are served by ``tiled.tiledAggregate(adj, dequantised T, edge_weight=)``. The first call on an
    adjacency builds its value index, which reads nnz back once: warm up before a capture."""
    tiled._check(adj_view)
    route = _check_route(route)
    bits = _check_bits(bits)
    if edge_weight is not None and (route != "bytes" or _check_reduce(reduce) != "sum"):
        raise ValueError(f'edge_weight needs route="bytes" and reduce="sum", not route={route!r}, reduce={reduce!r}')
    if _check_reduce(reduce) != "sum":
        if route != "bytes":
            raise ValueError(f'reduce="{reduce}" needs route="bytes": the planes route sums')
        if row_scale is not None:
            raise ValueError(f'row_scale cannot be combined with reduce="{reduce}"')
    coded = isinstance(T, torch.Tensor) and T.dtype == torch.uint8
    if route != "bytes" and (coded or t_qparams is not None or out is not None):
        raise ValueError('uint8 T, t_qparams= and out= need route="bytes"')
    if coded:
        T = _check_codes(adj_view, T, "T")
        if t_qparams is None:
            raise ValueError("uint8 T needs t_qparams, the row its codes were made under")
    else:
        _check_f32(T, "T")
    n, N = T.shape
    if n != adj_view.n or T.device != adj_view.device:
        raise ValueError(f"T must have shape [{adj_view.n}, N] on {adj_view.device}, not {list(T.shape)} on {T.device}")
    if row_scale is not None:
        tiled._check_scale(adj_view, row_scale)
    if t_qparams is not None:
        _check_qparams(t_qparams, "t_qparams", (1,), T)
    out_bits, out_qp = _check_out(out, T)
    if edge_weight is not None:
        tiled._check_edge_vector(adj_view, edge_weight, "edge_weight", T)
        heads = edge_weight.size(1) if edge_weight.dim() == 2 else 1
        if heads > 1 and (N // heads) % 4:
            raise ValueError(f"edge_weight has {heads} heads of {N // heads} columns: the byte-code walk needs a multiple of 4 columns a head; "
                             "tiled.tiledAggregate(adj, T, edge_weight=) on the dequantised T serves this shape")
    qt = qparams(T, bits) if t_qparams is None else t_qparams
    if route == "bytes":
        _check_masks(adj_view, row_mask, nbr_mask)
        Q = T if coded else codes(T, bits, qt)
        res, flt, mat, row = _dest(out, out_bits, out_qp, n, N, T.device)
        if edge_weight is not None:
            val_ptr, val_row, nnz = tiled._value_index(adj_view)
            index = (val_ptr.data_ptr(), val_row.data_ptr()) if adj_view.n_tiles else (None, None)
            _u8_call("affine.aggregate", "qgtc_tiledmm_u8", "_edge", adj_view, Q, row_mask, nbr_mask, qt.data_ptr(), _ptr(row_scale), *index,
                     edge_weight.data_ptr() if nnz else None, nnz, heads, *flt, *mat, *row)
        elif reduce != "sum":
            _u8_call("affine.aggregate", "qgtc_tiledmax_u8", "_affine", adj_view, Q, row_mask, nbr_mask, qt.data_ptr(), int(reduce == "min"),
                     *flt, *mat, *row)
        elif out is None:
            _u8_call("affine.aggregate", "qgtc_tiledmm_u8", "_affine", adj_view, Q, row_mask, nbr_mask, qt.data_ptr(), _ptr(row_scale), *flt)
        else:
            _u8_call("affine.aggregate", "qgtc_tiledmm_u8", "_requant", adj_view, Q, row_mask, nbr_mask, qt.data_ptr(), _ptr(row_scale),
                     *row, *mat)
        return res
    bit_T, _ = val2bit_affine(T, bits, qt, True, False)
    acc = QGTC.tiledMM2Int(adj_view, bit_T, N, bits, None, row_mask=row_mask, nbr_mask=nbr_mask)
    deg = adj_view.degrees(row_mask=row_mask, nbr_mask=nbr_mask)
    return dequant(acc, n, _identity_qparams(T.device), deg, qt, None, row_scale, out=acc)


def aggregate_linear(adj_view: "tiled.TiledAdjacency", T: torch.Tensor, t_qparams: torch.Tensor, h, W: torch.Tensor, w_bits: int,
                     per_column: bool = True, agg_row_scale=None, lin_row_scale=None, bias=None, relu: bool = False, row_mask=None,
                     nbr_mask=None, out=None) -> torch.Tensor:
    """The middle of the static chain in one launch (include/qgtc_fused.h): bit for bit
    ``linear(aggregate(adj_view, T, hb, agg_row_scale, row_mask, nbr_mask, route="bytes", t_qparams=t_qparams, out=h), W, hb, w_bits,
    per_column, lin_row_scale, bias, relu, route="bytes", x_qparams=h[1], out=out)`` with ``h = (hb, row)``, the intermediate never
    stored. T is uint8 [n, K], codes under ``t_qparams``; ``h`` the intermediate's fixed per-tensor row and its bits; W float32 [K, N2].
    ``out=(bits, row)`` gives uint8 codes [n, N2] (rows PAD16(N2) apart), otherwise float32 [n, N2]. :func:`pack_weight`, then the launch.
    The row view only, K and N2 up to ``FUSED_MAX``: anything else raises and names the two calls above, which serve it."""
    tiled._check(adj_view)
    two_calls = "; call aggregate(..., out=h) and then linear(..., x_qparams=h[1]) instead"
    if adj_view.transposed:
        raise ValueError("aggregate_linear has no fused kernel for the transposed view (adj.T)" + two_calls)
    T = _check_codes(adj_view, T, "T")
    n, K = T.shape
    if n != adj_view.n or T.device != adj_view.device:
        raise ValueError(f"T must have shape [{adj_view.n}, K] on {adj_view.device}, not {list(T.shape)} on {T.device}")
    _check_qparams(t_qparams, "t_qparams", (1,), T)
    h_bits, h_qp = _check_out(h, T)
    if h_qp is None:
        raise TypeError("h must be a tuple (bits, qparams row): the fixed row of the intermediate")
    w_bits = _check_bits(w_bits, "w_bits")
    _check_f32(W, "W")
    if W.size(0) != K or W.device != T.device:
        raise ValueError(f"W must have shape [{K}, N2] on {T.device}, not {list(W.shape)} on {W.device}")
    N2 = W.size(1)
    if K > FUSED_MAX or N2 > FUSED_MAX:
        raise ValueError(f"K = {K}, N2 = {N2}: the fused kernel holds widths up to {FUSED_MAX} in one workgroup" + two_calls)
    if agg_row_scale is not None:
        tiled._check_scale(adj_view, agg_row_scale)
    for t, name, m in ((lin_row_scale, "lin_row_scale", n), (bias, "bias", N2)):
        if t is not None:
            _check_vector(t, name, torch.float32, m, T)
    _check_masks(adj_view, row_mask, nbr_mask)
    out_bits, out_qp = _check_out(out, T)
    codes_t, qb, col_sums = pack_weight(W, w_bits, per_column)
    res, flt, mat, row = _dest(out, out_bits, out_qp, n, N2, T.device)
    _u8_call("affine.aggregate_linear", "qgtc_tiledmm_u8", "_linear", adj_view, T, row_mask, nbr_mask, t_qparams.data_ptr(),
             _ptr(agg_row_scale), h_qp.data_ptr(), h_bits, codes_t.data_ptr(), codes_t.size(1), codes_t.numel(), N2, qb.data_ptr(), qb.size(0),
             col_sums.data_ptr(), _ptr(lin_row_scale), _ptr(bias), int(bool(relu)), *flt, *mat, *row)
    return res


class GCNConv_Affine(torch.nn.Module):
    """The layer pair of ``conv.GCNConv`` on the bit-GEMM engine with affine quantisation:
    out = agg(linear(agg(linear(X, W_in)), W_out)), weights quantised per output column to ``w_bit`` bits, activations per tensor to
    ``act_bit`` bits, both at every forward from the values they hold then (nothing is cached, so a captured forward follows its
    parameters and inputs). ``norm`` is None (the plain sum), "mean" (``A.mean_scale()`` as the aggregate's row scale) or "sym"
    (D^-1/2 . A . D^-1/2: ``A.T.sym_scale()`` as the row scale of ``linear``, so the source factor is applied before the neighbour sum is
    quantised, and ``A.sym_scale()`` on the aggregate). ``A`` is a QGTC.TiledAdjacency view; X moves to its numbering and the result
    back. ``nodes`` (bool [n] in X's numbering) runs the pair on the induced subgraph: one bitmap as both masks, with the masked degrees
    and scales; rows outside come back +0. ``route`` ("planes" or "bytes") is the route of both aggregates (:func:`aggregate`; the same
    bits either way), ``linear_route`` that of both linear layers (:func:`linear`; likewise). ``aggr`` is the reducer of both aggregates,
    read at every forward like ``norm``: "sum", or "max" / "min", the twin of ``conv.GCNConv(aggr=...)`` on the extremum walks of
    include/qgtc_codes_max.h - with ``norm=None`` and ``route="bytes"`` only, anything else a ValueError. Inference only: forward runs
    without grad."""

    def __init__(self, input_dim, hidden_dim, output_dim, w_bit=4, act_bit=8, norm=None, route="planes", linear_route="planes", aggr="sum"):
        super().__init__()
        self.w_bit, self.act_bit = _check_bits(w_bit, "w_bit"), _check_bits(act_bit, "act_bit")
        self.norm = norm
        self.route = route
        self.linear_route = linear_route
        self.aggr = aggr
        self._check_config()
        self.W_in = torch.nn.Parameter(torch.randn(input_dim, hidden_dim))
        self.W_out = torch.nn.Parameter(torch.randn(hidden_dim, output_dim))

    def _check_config(self):
        if self.norm not in (None, "mean", "sym"):
            raise ValueError(f'norm must be None, "mean" or "sym", not {self.norm!r}')
        _check_bits(self.w_bit, "w_bit")
        _check_bits(self.act_bit, "act_bit")
        _check_route(self.route)
        if self.linear_route not in ROUTES:
            raise ValueError(f'linear_route must be "planes" or "bytes", not {self.linear_route!r}')
        if _check_reduce(self.aggr, "aggr") != "sum":
            if self.norm is not None:
                raise ValueError(f'aggr="{self.aggr}" takes no norm (norm={self.norm!r}): an extremum is not scaled')
            if self.route != "bytes":
                raise ValueError(f'aggr="{self.aggr}" needs route="bytes", not {self.route!r}: the planes route sums')

    @classmethod
    def from_float(cls, layer: "conv.GCNConv", w_bit: int = 4, act_bit: int = 8, route: str = "planes",
                   linear_route: str = "planes") -> "GCNConv_Affine":
        """The quantised twin of a (trained) float ``conv.GCNConv``: its two weights (copied), its norm and its aggr."""
        if not isinstance(layer, conv.GCNConv):
            raise TypeError(f"layer must be a conv.GCNConv, not {type(layer).__name__}")
        if layer.edge_drop > 0.0:
            raise ValueError(f"edge_drop={layer.edge_drop} has no quantised twin: the layer is inference only")
        new = cls(layer.W_in.size(0), layer.W_in.size(1), layer.W_out.size(1), w_bit, act_bit, layer.norm, route, linear_route,
                  layer.aggr)
        with torch.no_grad():
            new.W_in.copy_(layer.W_in)
            new.W_out.copy_(layer.W_out)
        return new.to(layer.W_in.device)

    def _operands(self, A, X, nodes):
        """(X in A's numbering, the mask keywords, the aggregate's row scale, the linear's) of one forward"""
        self._check_config()
        if not isinstance(A, QGTC.TiledAdjacency):
            raise NotImplementedError("GCNConv_Affine needs a QGTC.TiledAdjacency (QGTC.pack_edges_tiled), not a dense A")
        _check_f32(X, "X")
        if X.size(0) != A.n:
            raise ValueError(f"X must have one row per node ({A.n}), not shape {list(X.shape)}")
        mask = {}
        if nodes is not None:
            bm = conv._node_mask(A, nodes)
            mask = {"row_mask": bm, "nbr_mask": bm}
        row = src = None
        if self.norm == "mean":
            row = A.mean_scale(**mask)
        elif self.norm == "sym":
            row, src = A.sym_scale(**mask), A.T.sym_scale(**mask)
        return A.to_new(X).contiguous(), mask, row, src

    def _check_static(self):
        if self.route != "bytes" or self.linear_route != "bytes":
            raise ValueError(f'the static chain needs route="bytes" and linear_route="bytes", not {self.route!r} and {self.linear_route!r}')

    @torch.no_grad()
    def calibrate(self, A, X, nodes=None) -> torch.Tensor:
        """float32 [4, 4]: the qparams rows of the four activations of ``forward(A, X, nodes)`` - X in the adjacency's numbering and the
        outputs of the first linear, the first aggregate and the second linear -, exactly the rows the dynamic forward computes on the
        bytes routes: ``layer(A, X, act_qparams=layer.calibrate(A, X))`` is ``layer(A, X)`` bit for bit. Nothing is kept on the module."""
        self._check_static()
        Xn, mask, row, src = self._operands(A, X, nodes)
        W_in, W_out = self.W_in.detach().contiguous(), self.W_out.detach().contiguous()
        b = self.act_bit
        rows = [qparams(Xn, b)]
        t = linear(Xn, W_in, b, self.w_bit, True, src, route="bytes", x_qparams=rows[0])
        rows.append(qparams(t, b))
        h = aggregate(A, t, b, row, route="bytes", t_qparams=rows[1], reduce=self.aggr, **mask)
        rows.append(qparams(h, b))
        rows.append(qparams(linear(h, W_out, b, self.w_bit, True, src, route="bytes", x_qparams=rows[2]), b))
        return torch.cat(rows)

    @torch.no_grad()
    def forward(self, A, X, nodes=None, act_qparams=None, fuse=False):
        """``act_qparams`` (float32 [4, 4] on the device, as :meth:`calibrate` returns it) runs the static chain on the bytes routes
        (include/qgtc_chain.h): product float -> codes, walk codes -> codes, product codes -> codes, walk codes -> float32, each stage's
        output re-quantised in its producer's epilogue under the fixed rows; two ``pack_weight`` launches beside them, as now. ``fuse=True`` (with
        ``act_qparams`` only) runs the first walk and the second product as one launch (:func:`aggregate_linear`): five launches, the
        same bits."""
        Xn, mask, row, src = self._operands(A, X, nodes)
        W_in, W_out = self.W_in.detach().contiguous(), self.W_out.detach().contiguous()
        b = self.act_bit
        if fuse and act_qparams is None:
            raise ValueError("fuse=True needs act_qparams: only the static chain has a fused launch")
        if fuse and self.aggr != "sum":
            raise ValueError(f'fuse=True cannot be combined with aggr="{self.aggr}": the fused kernel sums; use fuse=False')
        red = {"reduce": self.aggr}
        if act_qparams is not None:
            self._check_static()
            _check_f32(act_qparams, "act_qparams")
            if tuple(act_qparams.shape) != (4, 4) or act_qparams.device != X.device:
                raise ValueError(f"act_qparams must have shape [4, 4] on {X.device}, not {list(act_qparams.shape)} on {act_qparams.device}")
            q0, q1, q2, q3 = (act_qparams[i:i + 1] for i in range(4))   # rows of a contiguous [4, 4]: 16-byte aligned views
            t = linear(Xn, W_in, b, self.w_bit, True, src, route="bytes", x_qparams=q0, out=(b, q1))
            if fuse:
                t = aggregate_linear(A, t, q1, (b, q2), W_out, self.w_bit, True, row, src, out=(b, q3), **mask)
                return A.to_old(aggregate(A, t, b, row, route="bytes", t_qparams=q3, **mask))
            h = aggregate(A, t, b, row, route="bytes", t_qparams=q1, out=(b, q2), **red, **mask)
            t = linear(h, W_out, b, self.w_bit, True, src, route="bytes", x_qparams=q2, out=(b, q3))
            return A.to_old(aggregate(A, t, b, row, route="bytes", t_qparams=q3, **red, **mask))
        lin = {"route": self.linear_route}
        h = aggregate(A, linear(Xn, W_in, b, self.w_bit, True, src, **lin), b, row, route=self.route, **red, **mask)
        return A.to_old(aggregate(A, linear(h, W_out, b, self.w_bit, True, src, **lin), b, row, route=self.route, **red, **mask))


class _AttentionConv_Affine(torch.nn.Module):
    """What the two quantised attention layers share. The projections run through ``linear(..., route="bytes")`` (weights per output
    column to ``w_bit`` bits, X per tensor to ``act_bit``), the scores and the edge softmax are the float launches of ``tiled`` on the
    projected features, and the value sum is ``aggregate(A, V, act_bit, route="bytes", edge_weight=alpha)``: V is gathered one byte an
    element. The head mean and ``to_new`` / ``to_old`` are the float layers'. ``nodes`` (bool [n] in X's numbering) is one bitmap as
    both masks of the value aggregate: rows outside come back +0 and neighbours outside add nothing. The softmax still normalises over
    ALL stored neighbours, so the masked layer is the aggregate restricted to the node set, not a softmax over the induced subgraph.
    Inference only: forward runs without grad. A subclass gives ``_project`` and ``_scores``."""

    def _init_common(self, input_dim, output_dim, heads, concat, w_bit, act_bit):
        if int(heads) < 1:
            raise ValueError(f"heads must be at least 1, not {heads!r}")
        self.input_dim, self.output_dim, self.heads, self.concat = int(input_dim), int(output_dim), int(heads), bool(concat)
        self.w_bit, self.act_bit = _check_bits(w_bit, "w_bit"), _check_bits(act_bit, "act_bit")

    def _weight(self):
        return torch.nn.Parameter(torch.randn(self.input_dim, self.heads * self.output_dim) / self.input_dim ** 0.5)

    def _linear(self, Xn, W):
        return linear(Xn, W.detach().contiguous(), self.act_bit, self.w_bit, route="bytes")

    @torch.no_grad()
    def forward(self, A, X, nodes=None):
        if not isinstance(A, QGTC.TiledAdjacency):
            raise NotImplementedError(f"{type(self).__name__} needs a QGTC.TiledAdjacency (QGTC.pack_edges_tiled), not a dense or edge-list A")
        _check_f32(X, "X")
        if X.size(0) != A.n:
            raise ValueError(f"X must have one row per node ({A.n}), not shape {list(X.shape)}")
        mask = {}
        if nodes is not None:
            bm = conv._node_mask(A, nodes)
            mask = {"row_mask": bm, "nbr_mask": bm}
        V, logits = self._scores(A, A.to_new(X).contiguous())
        out = aggregate(A, V, self.act_bit, route="bytes", edge_weight=tiled.tiledEdgeSoftmax(A, logits), **mask)
        if self.heads > 1 and not self.concat:   # the mean over the heads, in the layout and order of torch.stack(heads).mean(dim=0)
            out = out.view(A.n, self.heads, self.output_dim).transpose(0, 1).contiguous().mean(dim=0)
        return A.to_old(out)


class TransformerConv_Affine(_AttentionConv_Affine):
    """The quantised inference twin of ``conv.TransformerConv``: q, k, v = linear(X, W_q / W_k / W_v), the scores
    ``tiled.tiledEdgeScores(A, q, k, heads) / sqrt(output_dim)``, then the shared softmax and byte-code value sum."""

    def __init__(self, input_dim, output_dim, heads=1, concat=True, w_bit=4, act_bit=8):
        super().__init__()
        self._init_common(input_dim, output_dim, heads, concat, w_bit, act_bit)
        for name in ("W_q", "W_k", "W_v"):
            setattr(self, name, self._weight())

    @classmethod
    def from_float(cls, layer: "conv.TransformerConv", w_bit: int = 4, act_bit: int = 8) -> "TransformerConv_Affine":
        """The twin of a (trained) float layer: its three weights (copied), its heads and concat."""
        if not isinstance(layer, conv.TransformerConv):
            raise TypeError(f"layer must be a conv.TransformerConv, not {type(layer).__name__}")
        new = cls(layer.input_dim, layer.output_dim, layer.heads, layer.concat, w_bit, act_bit)
        with torch.no_grad():
            for name in ("W_q", "W_k", "W_v"):
                getattr(new, name).copy_(getattr(layer, name))
        return new.to(layer.W_q.device)

    def _scores(self, A, Xn):
        q, k, v = (self._linear(Xn, W) for W in (self.W_q, self.W_k, self.W_v))
        return v, tiled.tiledEdgeScores(A, q, k, self.heads) * (1.0 / math.sqrt(self.output_dim))


class GATv2Conv_Affine(_AttentionConv_Affine):
    """The quantised inference twin of ``conv.GATv2Conv``: hl = linear(X, W_l), hr = linear(X, W_r) (hl itself with ``share_weights``),
    the scores ``tiled.tiledEdgeAdditiveScores(A, hr, hl, att, negative_slope, heads)``, then the shared softmax and byte-code value sum
    of hl. ``att`` stays float32."""

    def __init__(self, input_dim, output_dim, heads=1, negative_slope=0.2, concat=True, share_weights=False, w_bit=4, act_bit=8):
        super().__init__()
        self._init_common(input_dim, output_dim, heads, concat, w_bit, act_bit)
        slope = float(negative_slope)
        if not 0.0 <= slope <= 1.0:
            raise ValueError(f"negative_slope must lie in [0, 1], not {negative_slope!r}")
        self.negative_slope, self.share_weights = slope, bool(share_weights)
        self.W_l = self._weight()
        if not self.share_weights:
            self.W_r = self._weight()
        self.att = torch.nn.Parameter(torch.randn(self.heads, self.output_dim) / self.output_dim ** 0.5)

    @classmethod
    def from_float(cls, layer: "conv.GATv2Conv", w_bit: int = 4, act_bit: int = 8) -> "GATv2Conv_Affine":
        """The twin of a (trained) float layer: its weights and ``att`` (copied), its heads, slope, concat and share_weights."""
        if not isinstance(layer, conv.GATv2Conv):
            raise TypeError(f"layer must be a conv.GATv2Conv, not {type(layer).__name__}")
        new = cls(layer.input_dim, layer.output_dim, layer.heads, layer.negative_slope, layer.concat, layer.share_weights, w_bit, act_bit)
        with torch.no_grad():
            for name in ("W_l", "att") + (() if layer.share_weights else ("W_r",)):
                getattr(new, name).copy_(getattr(layer, name))
        return new.to(layer.W_l.device)

    def _scores(self, A, Xn):
        hl = self._linear(Xn, self.W_l)
        hr = hl if self.share_weights else self._linear(Xn, self.W_r)
        return hl, tiled.tiledEdgeAdditiveScores(A, hr, hl, self.att.detach(), self.negative_slope, self.heads)
