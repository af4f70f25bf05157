"""Uniform affine quantisation on the bit-GEMM engine (include/qgtc_affine.h): x ~ scale * (q - zero_point), with
the range taken from the data on the device, so that real-valued features and trained weights run through ``bitMM2Int`` / ``tiledMM2Int``
and come back in real units. tests/affine_model.py states every bit of it in NumPy.

    qp = affine.qparams(x, bits)                          # float32 [G, 4]: (scale, zero_point, inv_scale, 0) per group, on the device
    words, sums = affine.val2bit_affine(x, bits, qp)      # the layouts of QGTC.val2bit(x, bits, col_major, False), and the code sums
    y = affine.dequant(acc, K, qa, row_sums, qb, col_sums)
    y = affine.linear(X, W, 8, 4)                         # ~ X @ W
    y = affine.aggregate(adj, T, 8)                       # ~ A . T on a QGTC.TiledAdjacency view
    y = affine.aggregate(adj, T, 8, route="bytes")        # the same bits from one walk over byte codes (include/qgtc_codes.h)
    q = affine.codes(x, bits, qp)                         # uint8 [H, W], one byte a code, rows PAD4(W) bytes apart
    acc = affine.tiledMMCodes(adj, q)                     # int32 [n, N]: the exact neighbour sum of the codes
    layer = affine.GCNConv_Affine.from_float(trained_gcnconv, 4, 8)

The C entries (four of include/qgtc_affine.h, five of include/qgtc_codes.h) are reached through ctypes on torch's current stream (the
extension binds no name for them): every call enqueues, reads nothing back and can be captured into a graph; the quantisation parameters stay on the device, so a replay follows the data's
range. The outputs and the scratch of the range launch are allocated here. Inference only: nothing here is differentiable, and no output
requires grad. The accumulators are float32 holding integers: ``linear`` refuses a K at which K * qmax_a * qmax_w could pass 2^24."""
from __future__ import annotations

import torch

import QGTC  # the HIP extension; there is no fallback

from . import conv, tiled
from .tiled import _c_abi, _ptr

__all__ = ["qparams", "val2bit_affine", "dequant", "linear", "aggregate", "GCNConv_Affine", "codes", "tiledMMCodes"]

ROUTES = ("planes", "bytes")   # how ``aggregate`` sums the codes: eight bit planes through tiledMM2Int, or one gather of byte codes

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


def linear(X: torch.Tensor, W: torch.Tensor, a_bits: int, w_bits: int, per_column: bool = True, row_scale=None, bias=None,
           relu: bool = False) -> torch.Tensor:
    """float32 [M, N] ~ X @ W on the bit-GEMM: X [M, K] quantised per tensor to ``a_bits`` (rows layout), W [K, N] per output column (or
    per tensor) to ``w_bits`` (cols layout, as ``GCNConv_Qnt.weight_Qnt`` packs weights), ``QGTC.bitMM2Int`` on the codes, then
    :func:`dequant` with the row sums of X's codes and the column sums of W's. Element [m][n] is within
    (sa / 2) sum_k |W[k][n]| + (sb[n] / 2) sum_k |X[m][k]| + K sa sb[n] / 4 of the exact product (to first order)."""
    a_bits, w_bits = _check_bits(a_bits, "a_bits"), _check_bits(w_bits, "w_bits")
    _check_f32(X, "X")
    _check_f32(W, "W")
    M, K = X.shape
    if W.size(0) != K or W.device != X.device:
        raise ValueError(f"W must have shape [{K}, N] on {X.device}, not {list(W.shape)} on {W.device}")
    N = W.size(1)
    if K * (2 ** a_bits - 1) * (2 ** w_bits - 1) >= 2 ** 24:
        raise ValueError(f"K = {K} at a_bits = {a_bits}, w_bits = {w_bits}: the float32 accumulator of bitMM2Int is exact below 2^24 only")
    qa = qparams(X, a_bits)
    bit_X, row_sums = val2bit_affine(X, a_bits, qa, False, True)
    qb = qparams(W, w_bits, per_column)
    bit_W, col_sums = val2bit_affine(W, w_bits, qb, True, True)
    acc = QGTC.bitMM2Int(bit_X, bit_W, M, K, N, a_bits, w_bits, True)   # pad_128: W's planes are PAD128(N) lines apart
    return dequant(acc, K, qa, row_sums, qb, col_sums, row_scale, bias, relu, out=acc)


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


def _check_codes(adj_view, Q) -> torch.Tensor:
    """Q as the C entries take it: any 2-D uint8 with unit column stride; a row stride or a base address off the 4-byte rule of a code
    matrix (include/qgtc_codes.h) gets a padded copy."""
    if not isinstance(Q, torch.Tensor):
        raise TypeError(f"Q must be a torch.Tensor, not {type(Q).__name__}")
    if Q.dtype != torch.uint8:
        raise TypeError(f"Q must be uint8, not {Q.dtype}")
    if not Q.is_cuda:
        raise ValueError(f"Q must be on a GPU, not on {Q.device}")
    if Q.dim() != 2:
        raise ValueError(f"Q must have 2 dimensions, not shape {list(Q.shape)}")
    if Q.numel() == 0:
        raise ValueError(f"Q must not be empty (shape {list(Q.shape)})")
    if Q.size(0) != adj_view.n or Q.device != adj_view.device:
        raise ValueError(f"Q must have shape [{adj_view.n}, N] on {adj_view.device}, not {list(Q.shape)} on {Q.device}")
    if Q.stride(1) != 1 and Q.size(1) > 1:
        raise ValueError(f"Q must have unit column stride, not strides {list(Q.stride())}")
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


def _u8_call(what: str, stem: str, adj_view, Q: torch.Tensor, out: torch.Tensor, row_mask, nbr_mask, *extra) -> torch.Tensor:
    fn = getattr(_c_abi(), stem + ("_t" if adj_view.transposed else "") + ("_affine" if extra else ""))
    _c_call(what, Q, fn, *tiled._view_args(adj_view), Q.data_ptr(), _codes_ld(Q), _codes_bytes(Q), Q.size(1), *extra, out.data_ptr(),
            out.numel(), _ptr(row_mask), _ptr(nbr_mask), adj_view.mask_words)
    return out


def tiledMMCodes(adj_view: "tiled.TiledAdjacency", Q: torch.Tensor, row_mask=None, nbr_mask=None) -> torch.Tensor:
    """int32 [n, N]: the exact sum of the code rows Q[k] (uint8 [n, N], in the adjacency's numbering) over the neighbours k of every row
    of the view ``adj_view`` (``adj`` or ``adj.T``), under the node masks of :func:`QGTC.tiledMM2Int` - what ``tiledMM2Int`` gives on the
    packed planes of the same codes, from one walk that gathers one dword of four codes per neighbour. One launch."""
    tiled._check(adj_view)
    Q = _check_codes(adj_view, Q)
    _check_masks(adj_view, row_mask, nbr_mask)
    out = torch.empty((adj_view.n, Q.size(1)), dtype=torch.int32, device=Q.device)
    return _u8_call("affine.tiledMMCodes", "qgtc_tiledmm_u8", adj_view, Q, out, row_mask, nbr_mask)


def aggregate(adj_view: "tiled.TiledAdjacency", T: torch.Tensor, bits: int, row_scale=None, row_mask=None, nbr_mask=None,
              route: str = "planes") -> torch.Tensor:
    """float32 [n, N] ~ A . T on the view ``adj_view`` (``adj`` or ``adj.T``; T in the adjacency's numbering): T quantised per tensor to
    ``bits`` into the cols layout, ``QGTC.tiledMM2Int`` on the codes (the exact neighbour sum), then :func:`dequant` with the view's
    degrees under the masks as the row sums of A, and ``row_scale`` (float32 [n], say ``adj_view.mean_scale()``) applied there. Row i is
    within deg_i * scale / 2 of the exact sum; a row without live neighbours, or outside ``row_mask``, comes back +0.

    ``route="bytes"`` gives the same bits from byte codes (include/qgtc_codes.h): :func:`qparams`, :func:`codes`,
    then one launch that gathers the neighbours' codes, counts the terms of every row and dequantises in its epilogue - four launches, no
    degree launch and no integer intermediate."""
    tiled._check(adj_view)
    route = _check_route(route)
    bits = _check_bits(bits)
    _check_f32(T, "T")
    n, N = T.shape
    if n != adj_view.n or T.device != adj_view.device:
        raise ValueError(f"T must have shape [{adj_view.n}, N] on {adj_view.device}, not {list(T.shape)} on {T.device}")
    if row_scale is not None:
        tiled._check_scale(adj_view, row_scale)
    qt = qparams(T, bits)
    if route == "bytes":
        _check_masks(adj_view, row_mask, nbr_mask)
        out = torch.empty((n, N), dtype=torch.float32, device=T.device)
        return _u8_call("affine.aggregate", "qgtc_tiledmm_u8", adj_view, codes(T, bits, qt), out, row_mask, nbr_mask, qt.data_ptr(),
                        _ptr(row_scale))
    bit_T, _ = val2bit_affine(T, bits, qt, True, False)
    acc = QGTC.tiledMM2Int(adj_view, bit_T, N, bits, None, row_mask=row_mask, nbr_mask=nbr_mask)
    deg = adj_view.degrees(row_mask=row_mask, nbr_mask=nbr_mask)
    return dequant(acc, n, _identity_qparams(T.device), deg, qt, None, row_scale, out=acc)


class GCNConv_Affine(torch.nn.Module):
    """The layer pair of ``conv.GCNConv`` on the bit-GEMM engine with affine quantisation:
    out = agg(linear(agg(linear(X, W_in)), W_out)), weights quantised per output column to ``w_bit`` bits, activations per tensor to
    ``act_bit`` bits, both at every forward from the values they hold then (nothing is cached, so a captured forward follows its
    parameters and inputs). ``norm`` is None (the plain sum), "mean" (``A.mean_scale()`` as the aggregate's row scale) or "sym"
    (D^-1/2 . A . D^-1/2: ``A.T.sym_scale()`` as the row scale of ``linear``, so the source factor is applied before the neighbour sum is
    quantised, and ``A.sym_scale()`` on the aggregate). ``A`` is a QGTC.TiledAdjacency view; X moves to its numbering and the result
    back. ``nodes`` (bool [n] in X's numbering) runs the pair on the induced subgraph: one bitmap as both masks, with the masked degrees
    and scales; rows outside come back +0. ``route`` ("planes" or "bytes") is the route of both aggregates (:func:`aggregate`; the same
    bits either way); ``linear`` stays on the bit-GEMM. Inference only: forward runs without grad."""

    def __init__(self, input_dim, hidden_dim, output_dim, w_bit=4, act_bit=8, norm=None, route="planes"):
        super().__init__()
        self.w_bit, self.act_bit = _check_bits(w_bit, "w_bit"), _check_bits(act_bit, "act_bit")
        self.norm = norm
        self.route = route
        self._check_config()
        self.W_in = torch.nn.Parameter(torch.randn(input_dim, hidden_dim))
        self.W_out = torch.nn.Parameter(torch.randn(hidden_dim, output_dim))

    def _check_config(self):
        if self.norm not in (None, "mean", "sym"):
            raise ValueError(f'norm must be None, "mean" or "sym", not {self.norm!r}')
        _check_bits(self.w_bit, "w_bit")
        _check_bits(self.act_bit, "act_bit")
        _check_route(self.route)

    @classmethod
    def from_float(cls, layer: "conv.GCNConv", w_bit: int = 4, act_bit: int = 8, route: str = "planes") -> "GCNConv_Affine":
        """The quantised twin of a (trained) float ``conv.GCNConv``: its two weights (copied) and its norm."""
        if not isinstance(layer, conv.GCNConv):
            raise TypeError(f"layer must be a conv.GCNConv, not {type(layer).__name__}")
        if layer.aggr != "sum":
            raise ValueError(f'aggr="{layer.aggr}" has no quantised twin: only aggr="sum" is built')
        if layer.edge_drop > 0.0:
            raise ValueError(f"edge_drop={layer.edge_drop} has no quantised twin: the layer is inference only")
        new = cls(layer.W_in.size(0), layer.W_in.size(1), layer.W_out.size(1), w_bit, act_bit, layer.norm, route)
        with torch.no_grad():
            new.W_in.copy_(layer.W_in)
            new.W_out.copy_(layer.W_out)
        return new.to(layer.W_in.device)

    @torch.no_grad()
    def forward(self, A, X, nodes=None):
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
        W_in, W_out = self.W_in.detach().contiguous(), self.W_out.detach().contiguous()
        h = aggregate(A, linear(A.to_new(X).contiguous(), W_in, self.act_bit, self.w_bit, True, src), self.act_bit, row, route=self.route,
                      **mask)
        return A.to_old(aggregate(A, linear(h, W_out, self.act_bit, self.w_bit, True, src), self.act_bit, row, route=self.route, **mask))
