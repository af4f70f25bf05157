"""NumPy model of the node reordering rule (include/qgtc.h, "Node reordering"; QGTC.reorder_nodes): size-capped label
propagation on the symmetrised graph, half the nodes a sweep, then the nodes sorted by (label, id). The GPU result must equal
it element for element. Also the tile count T of an edge list, the figure the reordering is for."""
import numpy as np

GOLDEN = 0x9E3779B9


def mix32(x):
    """lowbias32 on uint32 arrays."""
    x = np.asarray(x, dtype=np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x


def reorder_model(src, dst, n, sweeps=20, cap=128, return_sweeps=False):
    """(perm, rank) int64 [n]: perm[new] = old, rank[old] = new. Edges with an index outside [0, n) are skipped."""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    ok = (src >= 0) & (src < n) & (dst >= 0) & (dst < n) & (src != dst)
    u = np.concatenate([src[ok], dst[ok]])
    v = np.concatenate([dst[ok], src[ok]])
    ids = np.arange(n, dtype=np.int64)
    has = np.bincount(u, minlength=n) > 0
    label = ids.copy()
    quiet, ran = 0, 0
    for t in range(sweeps):
        ran += 1
        keys, cnt = np.unique(u * n + label[v], return_counts=True)
        x, lab = keys // n, keys % n
        h = mix32(lab.astype(np.uint32) ^ np.uint32((GOLDEN * (t + 1)) & 0xFFFFFFFF))
        order = np.lexsort((lab, h, -cnt, x))
        x, lab = x[order], lab[order]
        first = np.ones(x.size, dtype=bool)
        first[1:] = x[1:] != x[:-1]
        best = label.copy()
        best[x[first]] = lab[first]
        prop = np.where(has & ((ids + t) % 2 == 0), best, label)
        size = np.bincount(prop, minlength=n)
        new = np.where((prop == label) | (size[prop] <= cap), prop, label)
        changed = bool((new != label).any())
        label = new
        quiet = 0 if changed else quiet + 1
        if quiet >= 2:
            break
    perm = np.lexsort((ids, label)).astype(np.int64)
    rank = np.empty(n, dtype=np.int64)
    rank[perm] = ids
    return (perm, rank, ran) if return_sweeps else (perm, rank)


def tile_count(src, dst, n):
    """Occupied 32-row x 128-column tiles of the edge list's adjacency (cells of multiplicity 2 count as occupied: an upper bound
    of pack_edges_tiled's T, equal to it for edge lists without duplicates)."""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    nq = (n + 127) // 128
    return int(np.unique((src // 32) * nq + dst // 128).size)


def shuffled_sbm(n, deg=7.0, seed=3, shuffle_seed=7):
    """The issue's test graphs: make_sbm_graph(n, n // 128 blocks) and the same graph under a random relabelling."""
    from qgtc_ppopp22_amd.graph import make_sbm_graph

    g = make_sbm_graph("sbm", n, max(1, n // 128), deg, 1, seed=seed)
    p = np.random.default_rng(shuffle_seed).permutation(n)
    return g.src, g.dst, p[g.src], p[g.dst]
