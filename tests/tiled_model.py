"""Exact NumPy model of the tile-compressed adjacency (include/qgtc.h, "Tile-compressed adjacency" and "Transposed tiled adjacency";
QGTC.pack_edges_tiled, QGTC.tiledMM2Bit / tiledMM2Int on adj and adj.T): the format, the column index, and the products from the raw
edge list. The sums are exact int64; the expected words come from the C oracle's requant and rows-layout pack. No GPU."""
import numpy as np

# rows a thread owns in each product kernel, by output width N: the template variant the launchers pick
# (qgtc_tiled.hip, tiled_mm: `R = N <= 16 ? 2 : ...`; qgtc_tiled_t.hip, tiled_mm_t: `R = N <= 16 ? 8 : ...`)
FORWARD_VARIANTS = (2, 4, 8, 16)
TRANSPOSED_VARIANTS = (8, 16, 32, 64)


def variant(N, transposed):
    """R of k_tiled_mm (forward) or k_tiled_mm_t (transposed) at output width N."""
    v = TRANSPOSED_VARIANTS if transposed else FORWARD_VARIANTS
    return v[0] if N <= 16 else v[1] if N <= 32 else v[2] if N <= 64 else v[3]


def random_edges(rng, n, e):
    """Random edges with duplicates of multiplicity 2, 3 and 4, self loops, a hub row and a hub column; for n >= 96 row block 1
    (rows 32 .. 63) stays empty, and for n >= 512 k-quad 1 (columns 128 .. 255) too (below that the self loops of the hub row n // 2
    may fall into it)."""
    src = rng.integers(0, n, size=e, dtype=np.int64)
    dst = rng.integers(0, n, size=e, dtype=np.int64)
    if n > 2:
        src[: e // 8] = n // 2                     # a hub row
        dst[e // 8: e // 4] = n // 3               # a hub column
    if n >= 96:
        src = np.where((src >= 32) & (src < 64), src + 32, src)
    if n >= 384:
        dst = np.where((dst >= 128) & (dst < 256), dst + 128, dst)
    k = min(e, 16)
    dst[:k] = src[:k]                              # self loops
    if e:
        idx = rng.integers(0, e, size=max(1, e // 10))
        src = np.concatenate([src, src[idx], src[idx[::2]], src[idx[::4]]])
        dst = np.concatenate([dst, dst[idx], dst[idx[::2]], dst[idx[::4]]])
    return src, dst


def set_cells(src, dst, n):
    """The set cells of the 1-bit adjacency as sorted int64 keys row * n + col: in-range edges only, multiplicities 1, 2, >= 3
    quantised to 1, 0, 1, self loops kept."""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    ok = (src >= 0) & (src < n) & (dst >= 0) & (dst < n)
    cells, counts = np.unique(src[ok] * n + dst[ok], return_counts=True)
    return cells[(counts == 1) | (counts >= 3)]


def np_tiled(src, dst, n):
    """NumPy model of the format: (row_ptr int64, kquad int32, tiles uint32 [T, 32, 4])."""
    cells = set_cells(src, dst, n)
    r, c = cells // n, cells % n
    nrb, nq = (n + 31) // 32, (n + 127) // 128
    tile = (r // 32) * nq + c // 128
    uniq, inv = np.unique(tile, return_inverse=True)
    tiles = np.zeros((uniq.size, 32, 4), dtype=np.uint32)
    np.bitwise_or.at(tiles, (inv, r % 32, (c % 128) // 32), (np.uint32(1) << (31 - (c % 32)).astype(np.uint32)))
    row_ptr = np.zeros(nrb + 1, dtype=np.int64)
    row_ptr[1:] = np.cumsum(np.bincount(uniq // nq, minlength=nrb))
    return row_ptr, (uniq % nq).astype(np.int32), tiles


def np_colindex(row_ptr, kquad, n):
    """NumPy model of the column index: (col_ptr int64 [S128(n)+1], col_tile int64 [T], col_rb int32 [T])."""
    row_ptr, kquad = np.asarray(row_ptr, np.int64), np.asarray(kquad, np.int64)
    nq, T = (n + 127) // 128, kquad.size
    rb = np.repeat(np.arange(row_ptr.size - 1), np.diff(row_ptr))
    order = np.lexsort((np.arange(T), kquad))          # by k-quad, then tile id
    col_ptr = np.zeros(nq + 1, np.int64)
    col_ptr[1:] = np.cumsum(np.bincount(kquad, minlength=nq))
    return col_ptr, order.astype(np.int64), rb[order].astype(np.int32)


def aggregate(src, dst, n, Xq, transposed=False, budget=1 << 23):
    """Exact int64 sums [n, N] of the product with the quantised adjacency A of the edge list: forward C[u] = sum_v A[u, v] Xq[v],
    transposed C[v] = sum_u A[u, v] Xq[u]. Xq holds the quantised features (values 0 .. 2^bit2 - 1). The set cells' gathered rows
    are summed a few feature columns at a time, so that at most `budget` int64 values are gathered at once."""
    Xq = np.asarray(Xq)
    N = Xq.shape[1]
    cells = set_cells(src, dst, n)
    r, c = cells // n, cells % n
    out_row, in_row = (c, r) if transposed else (r, c)
    order = np.argsort(out_row, kind="stable")
    out_row, in_row = out_row[order], in_row[order]
    C = np.zeros((n, N), dtype=np.int64)
    if cells.size == 0:
        return C
    starts = np.flatnonzero(np.r_[True, out_row[1:] != out_row[:-1]])
    step = max(1, budget // cells.size)
    for j0 in range(0, N, step):
        j1 = min(N, j0 + step)
        C[out_row[starts], j0:j1] = np.add.reduceat(Xq[in_row, j0:j1].astype(np.int64), starts, axis=0)
    return C


def requant(oracle, C, ob):
    """The oracle's requant of every sum (a float compare against 2^ob), as int32; each distinct sum is asked once."""
    vals, inv = np.unique(np.asarray(C, dtype=np.int64), return_inverse=True)
    assert vals.size == 0 or (vals.min() >= 0 and vals.max() < 2 ** 31)
    q = np.array([oracle.requant(int(v), ob) for v in vals], dtype=np.int32)
    return q[inv].reshape(np.shape(C))


def expected_bits(oracle, C, ob):
    """The rows-layout words [ob][PAD8(n)][S128(N)*4] (flat uint32) of requant(C): what tiledMM2Bit must give."""
    return oracle.pack(requant(oracle, C, ob), ob)


def expected_floats(C):
    """What tiledMM2Int must give: the sums as float32 [n, N]."""
    return np.asarray(C).astype(np.float32)
