"""Node masks on the quantised tiled products (include/qgtc_bitnodes.h): what ``tiled.tiledMM2Bit`` /
``tiled.tiledMM2Int`` do when they are given ``row_mask=`` / ``nbr_mask=``. The four C entries ``qgtc_tiledmm2bit_nodes`` /
``qgtc_tiledmm2int_nodes`` and their ``_t`` are reached through ctypes on the current stream (the extension binds no name for them), so a
masked call enqueues one launch, reads nothing back and can be captured into a graph. Nothing here is exported: the public names are
the two functions of ``tiled``, which delegate here only when a mask is given."""
from __future__ import annotations

import torch

from . import tiled


def _check_bits(adj: "tiled.TiledAdjacency", bit_X, N: int, bit2: int) -> None:
    """What the binding of the plain call checks of bit_X, with its exception types (TORCH_CHECK raises RuntimeError)."""
    if not isinstance(bit_X, torch.Tensor):
        raise TypeError("bit_X must be a torch.Tensor (val2bit(X, bit2, True, False))")
    if not bit_X.is_cuda:
        raise RuntimeError("bit_X must be a CUDA tensor")
    if not bit_X.is_contiguous():
        raise RuntimeError("bit_X must be contiguous")
    if bit_X.dtype != torch.int32:
        raise RuntimeError("bit_X must be an int32 bit tensor")
    if bit_X.device != adj.device:
        raise RuntimeError("the adjacency and bit_X must be on the same device")
    if N < 1 or not 1 <= bit2 <= 8:
        raise RuntimeError("bad dimensions")
    if bit_X.numel() < bit2 * ((N + 127) // 128 * 128) * adj.mask_words:
        raise RuntimeError("bit_X must hold bit2 x PAD128(N) x S128(n)*4 words (val2bit(X, bit2, True, False))")


def masked(adj: "tiled.TiledAdjacency", bit_X: torch.Tensor, N: int, bit2: int, output_bit: int, to_float: bool, row_scale,
           row_mask, nbr_mask) -> torch.Tensor:
    """The masked product on the view of ``adj``: rows-layout words [output_bit * PAD8(n), S128(N) * 4], or float32 [n, N] with
    ``to_float``. ``row_scale`` has been checked by the caller; at least one mask is given."""
    N, bit2, output_bit = int(N), int(bit2), int(output_bit)
    for mask, name in ((row_mask, "row_mask"), (nbr_mask, "nbr_mask")):
        if mask is not None:
            tiled._check_mask(adj, mask, name)
    _check_bits(adj, bit_X, N, bit2)
    n, T = adj.n, adj.n_tiles
    # the index array the kernels read even without tiles (row_ptr / col_ptr) is always passed; the others only with tiles
    if adj.transposed:
        view = (adj.col_ptr.data_ptr(),) + tuple(t.data_ptr() if T else None for t in (adj.col_tile, adj.col_rb, adj.tiles))
    else:
        view = (adj.row_ptr.data_ptr(),) + tuple(t.data_ptr() if T else None for t in (adj.kquad, adj.tiles))
    L = tiled._c_abi()
    tail = (tiled._ptr(row_scale),)
    if to_float:
        out = torch.empty((n, N), dtype=torch.float32, device=bit_X.device)
        fn, what = (L.qgtc_tiledmm2int_t_nodes if adj.transposed else L.qgtc_tiledmm2int_nodes), "tiledMM2Int (node masks)"
    else:
        if not 1 <= output_bit <= 32:
            raise RuntimeError("bad dimensions")
        out = torch.empty((output_bit * ((n + 7) // 8 * 8), (N + 127) // 128 * 4), dtype=torch.int32, device=bit_X.device)
        fn, what = (L.qgtc_tiledmm2bit_t_nodes if adj.transposed else L.qgtc_tiledmm2bit_nodes), "tiledMM2Bit (node masks)"
        tail = (output_bit,) + tail
    tiled._c_call(what, bit_X, fn, *view, T, n, bit_X.data_ptr(), bit_X.numel(), N, bit2, *tail, out.data_ptr(), out.numel(),
                  tiled._ptr(row_mask), tiled._ptr(nbr_mask), adj.mask_words)
    return out
