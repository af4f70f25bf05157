"""Tile-compressed 1-bit adjacency of a whole graph (include/qgtc.h, "Tile-compressed adjacency"; DESIGN.md sections 4, 6.10).

The dense route packs an n x n adjacency into n^2/8 bytes and stops at n = 185 363 (4 GiB per packed operand). A
:class:`TiledAdjacency` keeps only the occupied 32-row x 128-column tiles, block-sparse like BSR, and
:func:`tiledMM2Bit` / :func:`tiledMM2Int` multiply from that storage: word for word what ``bitMM2Bit`` / ``bitMM2Int`` give
on ``pack_edges(src, dst, n, n, 1)`` of the same edge list. ``QGTC`` re-exports the three functions and the class.
"""
from __future__ import annotations

import torch

from . import load_ext

_ext = load_ext()

__all__ = ["TiledAdjacency", "pack_edges_tiled", "tiledMM2Bit", "tiledMM2Int"]


class TiledAdjacency:
    """One-plane n x n adjacency as its occupied tiles (device tensors):

    ``row_ptr`` int64 [S32(n) + 1]: the tiles of 32-row block rb are ``row_ptr[rb] .. row_ptr[rb+1] - 1``;
    ``kquad`` int32 [T]: the 128-column group of each tile, strictly ascending within a row block;
    ``tiles`` int32 words [T, 32, 4]: row r of the block, the tile's 4 words of that row (element i at word i>>5, bit 31-(i&31)).
    """

    def __init__(self, n: int, row_ptr: torch.Tensor, kquad: torch.Tensor, tiles: torch.Tensor):
        self.n = int(n)
        self.row_ptr, self.kquad, self.tiles = row_ptr, kquad, tiles
        self._max_block_tiles = None

    @property
    def n_tiles(self) -> int:
        return int(self.kquad.numel())

    @property
    def device(self) -> torch.device:
        return self.row_ptr.device

    @property
    def nbytes(self) -> int:
        """Bytes of the three tensors (512 a tile, 4 a k-quad index, 8 a row block)."""
        return sum(t.numel() * t.element_size() for t in (self.row_ptr, self.kquad, self.tiles))

    @property
    def max_block_tiles(self) -> int:
        """Most tiles in one 32-row block (one host read, on first use)."""
        if self._max_block_tiles is None:
            self._max_block_tiles = int((self.row_ptr[1:] - self.row_ptr[:-1]).max().item()) if self.row_ptr.numel() > 1 else 0
        return self._max_block_tiles

    def to_rows(self) -> torch.Tensor:
        """The dense rows-layout words [PAD8(n), S128(n)*4] (what ``pack_edges(src, dst, n, n, 1)`` returns). A test aid for small n."""
        n = self.n
        nrb, nq = (n + 31) // 32, (n + 127) // 128
        dense = torch.zeros((nrb * 32, nq, 4), dtype=torch.int32, device=self.device)
        if self.n_tiles:
            rb = torch.repeat_interleave(torch.arange(nrb, device=self.device), self.row_ptr[1:] - self.row_ptr[:-1])
            rows = rb[:, None] * 32 + torch.arange(32, device=self.device)[None, :]
            dense[rows, self.kquad.long()[:, None].expand(-1, 32)] = self.tiles
        return dense[: (n + 7) // 8 * 8].reshape((n + 7) // 8 * 8, nq * 4).contiguous()

    def __repr__(self) -> str:
        return f"TiledAdjacency(n={self.n}, n_tiles={self.n_tiles}, nbytes={self.nbytes})"


def pack_edges_tiled(src: torch.Tensor, dst: torch.Tensor, n: int, validate: bool = True) -> TiledAdjacency:
    """Tile-compressed adjacency of the raw edge list (src[i] -> row, dst[i] -> column; duplicates allowed: multiplicities
    1, 2, >= 3 quantise to 1, 0, 1 as in ``pack_edges``). ``validate`` raises on an out-of-range or negative index;
    without it such edges are skipped."""
    row_ptr, kquad, tiles = _ext._tiled_pack(src, dst, int(n), bool(validate))
    return TiledAdjacency(n, row_ptr, kquad, tiles)


def _check(adj) -> None:
    if not isinstance(adj, TiledAdjacency):
        raise TypeError("adj must be a TiledAdjacency (QGTC.pack_edges_tiled)")


def tiledMM2Bit(adj: TiledAdjacency, bit_X: torch.Tensor, N: int, bit2: int, output_bit: int) -> torch.Tensor:
    """requant(A . X) in the rows layout [output_bit * PAD8(n), S128(N)*4]: ``bitMM2Bit(A_rows, bit_X, n, n, N, 1, bit2,
    output_bit)``. bit_X: cols layout [bit2][PAD128(N)][S128(n)*4] (``val2bit(X, bit2, True, False)`` / ``bitMM2Bit_col``)."""
    _check(adj)
    return _ext._tiled_mm(adj.row_ptr, adj.kquad, adj.tiles, adj.n, bit_X, int(N), int(bit2), int(output_bit), False)


def tiledMM2Int(adj: TiledAdjacency, bit_X: torch.Tensor, N: int, bit2: int) -> torch.Tensor:
    """float32 [n, N] = A . X: ``bitMM2Int(A_rows, bit_X, n, n, N, 1, bit2, True)``."""
    _check(adj)
    return _ext._tiled_mm(adj.row_ptr, adj.kquad, adj.tiles, adj.n, bit_X, int(N), int(bit2), 1, True)
