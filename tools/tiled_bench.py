"""Measure the tile-compressed whole-graph adjacency (QGTC.pack_edges_tiled + tiledMM2Bit) on SBM graphs of public-dataset size.

Per graph, as generated (block-local numbering), under a random node permutation, and that permutation renumbered on the device
(`reordered`: QGTC.reorder_nodes with its defaults, then pack_edges_tiled(..., reorder=True); reorder_ms is the reordering alone):
pack time, occupied tiles T, tile bytes, and the aggregate requant(A . X) (rows-layout output, ob = w) at N in {16, 64, 256} and
w in {1, 2, 4}, with the HBM fraction of the algorithmic bytes (512 T + 12 T + X + out) against 8 TB/s. At the arxiv size also the dense route (pack_edges + bitMM2Bit).

`--leg transposed` measures A^T . X instead, on the reordered graphs and on an arxiv-sized graph whose in-degree
follows a power law (`arxiv-skew`: half the edges point at Zipf-drawn nodes): the column index build (`adj.T`) and its bytes, the
reversed pack a user would do without it (`pack_edges_tiled(rank[dst], rank[src], n)`), and tiledMM2Bit at N in {16, 64, 256} and
w in {1, 2} (ob = w) on adj.T, on that reverse-packed adjacency and forward on adj (the first two checked equal).

`--leg scaled` measures the scaled products and the degrees on the reordered graphs, both directions, N in
{16, 64, 256}, w in {1, 2}, ob = w, with the mean scale: (a) tiledMM2Bit with and without row_scale, the two launched alternately in
one timed loop, and with a scale of ones (the unscaled words through the scaled kernels); (b) the degrees call (both directions and both reciprocals: the first `degrees()` / `mean_scale()`); (c) the route
without the feature - tiledMM2Int, a float multiply by the scale, val2bit - checked equal to (a). Each figure is the median of the
per-launch event times with their 10th and 90th percentiles. It also counts, on the device, the share of in-neighbour outputs at
the clamp value 2^b - 1 for the plain sum and for the mean at 2 / 3 / 4 bits (N = 64, random features over the full range).

`--leg float` measures the float products (QGTC.tiledMMFloat) on the reordered graphs, both directions, N in
{16, 64, 256}, launched alternately in one timed loop with (a) tiledMMFloat with the mean scale, (b) the only comparable route without
the feature, tiledMM2Int on the 8 bit planes of the same matrix (integers 0 .. 255, so the two agree bit for bit: checked), and (c)
that route with its val2bit inside the clock. Reported with the traffic floor of the float product - (set cells x N x 4 bytes of X
rows + n x N x 4 bytes written + 524 bytes a tile) / 8 TB/s - as a fraction of the measured time.

`--leg sym` measures the source scale and the differentiable aggregate (QGTC.tiledMMFloat(src_scale=), QGTC.tiledAggregate; DESIGN.md
6.15) on the reordered graphs, both directions, N in {16, 64, 256}, standard-normal X, with the symmetric normalisation
(row_scale = sym_scale() of the view, src_scale = that of the other view), launched alternately in one timed loop: (a) tiledMMFloat with
the row scale only, (b) with both scales in one launch, (c) the route without the feature, tiledMMFloat(adj, X * c[:, None], r)
(checked bit-equal to (b) before timing), (d) forward plus backward of one tiledAggregate. Medians with their 10th and 90th
percentiles, and the ratios (b) / (a), (b) / (c), (d) / (b).

`--leg max` measures the extremum products (QGTC.tiledMMFloat(reduce="max"), QGTC.tiledAggregate(reduce="max")) on the
reordered graphs, both directions, N in {64, 256}, standard-normal X, launched alternately in one timed loop: (a) the float sum launch
tiledMMFloat(a, X), the comparison at the same shape, (b) the forward max without and (c) with the winners written, (d) the select alone
on the other view, (e) forward plus backward of one tiledAggregate(reduce="max"). Medians with their 10th and 90th percentiles, and the
ratios (b) / (a), (c) / (a), (d) / (a), (e) / (c). The winners are checked against a gather of X before timing.

`--leg attn` measures the attention products (QGTC.tiledMMFloat(attn=), QGTC.tiledAggregate(attn=)) on the reordered
graphs, both directions, N in {64, 256}, standard-normal X and scores, launched alternately in one timed loop: (a) the `sym` float launch
tiledMMFloat(a, X, r, c), the comparison at the same shape, (b) the attention forward (the N = 1 max launch plus the product launch),
(c) forward plus backward of tiledAggregate(attn=) for all three gradients, (d) forward plus backward of the `sym` tiledAggregate, and
the route without the feature, a torch edge-list scatter-softmax (amax and index_add_ with atomics, an [E, N] intermediate), (e) forward
and (f) forward plus backward; (b) is checked close to (e) before timing. Medians with their 10th and 90th percentiles, and the ratios
(b) / (a), (c) / (d), (e) / (b), (f) / (c).

`--leg drop` measures edge dropout inside the tile walk (``edge_drop=`` of QGTC.tiledMMFloat / QGTC.tiledAggregate) on the
reordered graphs, both directions, N in {64, 256}, standard-normal X and scores, in two alternating loops. First: (a) the plain sum
launch tiledMMFloat(a, X), (b) the masked launch at rates 0.1 and 0.5, (c) the route it replaces at rate 0.1 - filter the edge list with
a random mask (`torch.rand`: the same rate, not the same cells as the masked launch, which does not matter for a time), pack_edges_tiled,
(on adj.T: build the column index,) plain launch. Second, (d): forward plus backward of tiledAggregate
for the sum with `sym` scales, max and attention, each without the mask and with it at rate 0.1. The masked sum is checked bit-equal to
the plain launch on the adjacency packed from the kept cells before timing. Medians with their 10th and 90th percentiles, and the ratios
(b) / (a), (b) / (c) and masked / plain of (d).

`--leg nodes` measures node masks inside the tile walk (``row_mask=`` / ``nbr_mask=`` of QGTC.tiledMMFloat / QGTC.tiledAggregate;
DESIGN.md 6.15e) on the reordered graphs, both directions, N in {64, 256}, standard-normal X, under four node sets in the adjacency's
numbering: (i) a contiguous eighth of the ids, (ii) a random eighth of the 128-id communities, (iii) a random eighth of the nodes - the
worst case, every block stays live -, each as row and neighbour mask at once (the induced subgraph), and (iv) a random half of the nodes
as the row mask alone. Three alternating loops: first (a) the plain launch, the four masked launches and (c) the masked launch with
all-ones bitmaps; second (b), the route each masked launch replaces - filter the edge list by the two sets, pack_edges_tiled, (on adj.T:
build the column index,) plain launch; third, forward plus backward of tiledAggregate with `sym` scales, plain and under (i) - (iii).
Every masked sum is checked bit-equal to the plain launch on the re-packed adjacency before timing. Medians with their 10th and 90th
percentiles, the share of live workgroups of each mask, and the ratios masked / (a) and masked / (b).

`--leg edge` measures the edge values (``edge_weight=`` of QGTC.tiledMMFloat / QGTC.tiledAggregate, tiled.tiledSDDMM) on
the reordered graphs, both directions, N in {64, 256}, standard-normal X and weights. One alternating loop: the weighted launch, the
``src_scale`` launch of the same shape (the same multiply and add per term: the weighted launch adds 4 bytes an edge and 72 bytes a
tile of traffic), the plain launch, tiledSDDMM, the attention's grad_own launch (the same walk and dot, folded instead of stored),
forward plus both gradients of tiledAggregate(edge_weight=), and the edge-list route (index_select, multiply, index_add_ with its
autograd backward, which is not bit-reproducible). Once per graph: the value index plus edge_slots of the whole edge list against
pack_edges_tiled. The weighted sum is checked against the edge-list route before timing. Medians with their 10th and 90th percentiles.

`--leg esoftmax` measures the edge softmax (tiled.tiledEdgeSoftmax and its gradient, tiled.tiledEdgeAttention) on the
reordered graphs, both directions, d = N in {64, 256}, logits 3 * standard normal. Two alternating loops: first the softmax launch, its
gradient launch, tiledSDDMM and the weighted launch of the same shape, each alone; second tiledEdgeAttention forward and forward plus
all three gradients against the edge-list route (index_select, a row dot, scatter_reduce amax, exp, index_add_ twice, with its
autograd backward, which is not bit-reproducible). The attention is checked against the edge-list route before timing. Medians with
their 10th and 90th percentiles.

`--leg heads` measures multi-head attention in one call (tiled.tiledEdgeAttention(heads=H)) against the loop over the
heads it replaces - per head three `.contiguous()` column slices and the single-head call, concatenated -, on the reordered graphs
(arxiv and reddit unless --graphs says otherwise), both directions, (H, d) in {(8, 8), (4, 16), (8, 32), (4, 64)} for Q, K and V alike.
One alternating loop of four: forward and forward plus all three gradients, each way. Output and gradients of the two routes are
checked bit for bit before timing. Medians with their 10th and 90th percentiles; `within_spread` says whether the one-call median is at
most the loop's median plus the loop's own 10th-to-90th-percentile spread.

`--leg gatv2` measures the additive edge score of GATv2 (tiled.tiledEdgeAdditiveScores, tiled.tiledEdgeAdditiveAttention; DESIGN.md
6.15k) on the heads leg's graphs and (H, d) cells, both directions. Three alternating loops: the score launch against the
tiledSDDMM(heads=H) launch of the same shape; each gradient launch against the edge_weight weighted launch of the same shape and view;
the attention's forward and forward plus all four gradients against the edge-list route in torch (edge_endpoints, index_select,
leaky_relu, a scatter softmax, index_add_), against which it is checked before timing. Medians with their 10th and 90th percentiles; a
cell slower than the edge-list route is reported as such.

`--leg fanout` measures fixed-fanout neighbour sampling inside the tile walk (``fanout=`` of QGTC.tiledMMFloat / QGTC.tiledAggregate,
fanout.sample_fanout) on the reordered graphs, N in {64, 256}, k in {5, 10, 25}, both views: the selection launch, the
sampled sum in the own form (a sample of the view) and in the nbr form (a sample of the other view), forward plus backward, against (a)
the route without it - random keys on tiled.edge_endpoints, a per-row top-k in torch, pack_edges_tiled, the plain launch -, (b) the
plain launch and (c) the ``edge_drop`` launch at the rate that keeps as many edges.

`--leg blocks` measures mini-batch sampling (fanout.sample_blocks, fanout.frontier, ``sample_fanout(..., row_mask=)``) on
the reordered graphs, on adj, 1024 seed nodes, fanouts (25, 10), N in {64, 256}: (a) building the two blocks plus the two sampled mean
aggregates against today's route for the same batch - per hop, filter the edge list by the row set, a per-row top-k in torch,
pack_edges_tiled, the plain mean launch, the next row set by a scatter -, (b) the frontier launch against the three-launch route (the
N = 1 sampled product of ones on the other view, a compare, node_bitmap) and (c) the masked selection against the unmasked one.

`--leg bitnodes` measures node masks on the quantised products (``row_mask=`` / ``nbr_mask=`` of QGTC.tiledMM2Bit) on
the reordered graphs (pass --graphs arxiv,reddit), both directions, N = 64, 1 and 2 feature bits (output bits alike), under the node sets
of `--leg nodes`: a contiguous eighth, a community-aligned eighth and a random eighth, each as both masks, and a random half as the row
mask alone. Two alternating loops: first the plain launch, the four masked launches and the masked launch with all-ones bitmaps; second
the route each masked launch replaces - filter the edge list, pack_edges_tiled, (on adj.T: build the column index,) plain launch. Every
masked product is checked equal to the plain launch on the re-packed adjacency before timing. Medians with their 10th and 90th
percentiles, the share of live workgroups, and the ratios masked / plain and masked / re-pack.

`--leg affine` measures affine quantisation (qgtc_ppopp22_amd/affine.py) on the reordered graphs at N = 64: the range
launch, ``val2bit_affine`` in both layouts at 2 / 4 / 8 bits beside ``QGTC.val2bit`` at the same shape, ``dequant``, ``aggregate`` beside
``tiledMM2Int`` alone and ``tiledMMFloat``, the layer's forward beside ``conv.GCNConv``'s and its relative error against the float layer.

`--leg codes` measures the byte-code route (include/qgtc_codes.h) on the reordered graphs at N = 64 and 256, on adj and
adj.T: ``affine.codes`` beside ``val2bit_affine`` (cols, 8 bits), ``tiledMMCodes``, ``aggregate`` on both routes at 2 / 4 / 8 bits in the
same alternating rounds beside ``tiledMMFloat``, and the layer on both routes beside ``conv.GCNConv``. A cell passes (4 and 8 bits only)
when the bytes route's 90th percentile lies under the planes route's 10th.

    python tools/tiled_bench.py [--graphs arxiv,reddit,products] [--reps 10] [--json OUT] [--leg orders|transposed|scaled|float|sym|max|attn|drop|nodes|edge|esoftmax|heads|gatheads|gatv2|fanout|blocks|bitnodes|affine|codes]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRAPHS = {  # name -> (nodes, average out-degree)
    "arxiv": (169343, 7.0),
    "reddit": (232965, 20.0),
    "products": (2449029, 25.0),
}
HBM_BPS = 8e12


def timed(torch, fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))   # ms


def transposed_leg(torch, QGTC, graphs, reps):
    from qgtc_ppopp22_amd import tiled
    from qgtc_ppopp22_amd.graph import make_sbm_graph

    rows = []
    for name in graphs:
        base = name.split("-")[0]
        n, deg = GRAPHS[base]
        g = make_sbm_graph(base, n, max(1, n // 128), deg, 1, seed=3)
        rng = np.random.default_rng(7)
        perm = rng.permutation(n)
        src, dst = g.src, g.dst
        if name.endswith("-skew"):
            hubs = rng.permutation(n)
            zipf = hubs[(rng.zipf(1.6, size=dst.size) - 1) % n]
            dst = np.where(rng.random(dst.size) < 0.5, zipf, dst)
        dsrc, ddst = torch.from_numpy(perm[src]).cuda(), torch.from_numpy(perm[dst]).cuda()
        adj = QGTC.pack_edges_tiled(dsrc, ddst, n, reorder=True)
        rs, rd = adj.rank.index_select(0, dsrc), adj.rank.index_select(0, ddst)
        index_ms = timed(torch, lambda: tiled._ext._tiled_colindex(adj.row_ptr, adj.kquad, n), reps, warmup=2)
        rev_pack_ms = timed(torch, lambda: QGTC.pack_edges_tiled(rd, rs, n, False), reps, warmup=2)
        t = adj.T
        rev = QGTC.pack_edges_tiled(rd, rs, n)
        rec = {"graph": name, "order": "reordered", "n": n, "edges": int(src.size), "tiles": adj.n_tiles, "rev_tiles": rev.n_tiles,
               "index_ms": round(index_ms, 4), "index_bytes": t.nbytes - adj.nbytes, "rev_pack_ms": round(rev_pack_ms, 4),
               "rev_bytes": rev.nbytes, "max_block_tiles": adj.max_block_tiles, "max_col_tiles": t.max_block_tiles, "agg": []}
        print(f"{name:12s} T={adj.n_tiles} index {index_ms:.4f} ms ({rec['index_bytes']} B), reversed pack {rev_pack_ms:.4f} ms "
              f"({rev.nbytes} B), longest row list {adj.max_block_tiles}, longest column list {t.max_block_tiles}", flush=True)
        xr = np.random.default_rng(1)
        for N in (16, 64, 256):
            for w in (1, 2):
                X = QGTC.val2bit(torch.from_numpy(xr.integers(0, 2 ** w, size=(n, N)).astype(np.float32)).cuda(), w, True, False)
                assert torch.equal(QGTC.tiledMM2Bit(t, X, N, w, w), QGTC.tiledMM2Bit(rev, X, N, w, w))
                ms_t = timed(torch, lambda: QGTC.tiledMM2Bit(t, X, N, w, w), reps)
                ms_r = timed(torch, lambda: QGTC.tiledMM2Bit(rev, X, N, w, w), reps)
                ms_f = timed(torch, lambda: QGTC.tiledMM2Bit(adj, X, N, w, w), reps)
                rec["agg"].append({"N": N, "w": w, "transposed_ms": round(ms_t, 4), "reverse_packed_ms": round(ms_r, 4),
                                   "forward_ms": round(ms_f, 4), "t_over_rev": round(ms_t / ms_r, 3)})
                print(f"{name:12s} N={N:<4d} w={w} A^T.X {ms_t:8.4f} ms  reverse-packed {ms_r:8.4f} ms  forward {ms_f:8.4f} ms  "
                      f"ratio {ms_t / ms_r:.2f}", flush=True)
                del X
        rows.append(rec)
        del adj, t, rev, dsrc, ddst, rs, rd
        torch.cuda.empty_cache()
    return rows


def timed_alternating(torch, fns, reps, warmup=3):
    """Several callables launched in turn inside one loop, so that drift of the clocks or of a shared machine hits them alike; the
    order changes from round to round through every permutation (strided, so that few rounds still spread over all of them), so that
    each follows each other equally often (a launch inherits the caches its predecessor leaves). Per callable (median, 10th percentile,
    90th percentile) of the per-launch event times, ms."""
    import itertools

    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    orders = list(itertools.permutations(range(len(fns))))
    # itertools lists the permutations in lexicographic order: taken as they come, ten rounds of five callables would all start with
    # the same two. A stride coprime to their number spreads any count of rounds over the whole list and still visits every order.
    stride = next(k for k in range(max(1, round(len(orders) * 0.382)), 2 * len(orders) + 2) if math.gcd(k, len(orders)) == 1)
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in fns] for _ in range(reps)]
    for r, row in enumerate(ev):
        for k in orders[r * stride % len(orders)]:
            a, b = row[k]
            a.record()
            fns[k]()
            b.record()
    torch.cuda.synchronize()
    out = []
    for k in range(len(fns)):
        t = np.array([row[k][0].elapsed_time(row[k][1]) for row in ev])
        out.append(tuple(round(float(v), 4) for v in (np.median(t), np.percentile(t, 10), np.percentile(t, 90))))
    return out


def scaled_leg(torch, QGTC, graphs, reps):
    from qgtc_ppopp22_amd import tiled
    from qgtc_ppopp22_amd.graph import make_sbm_graph

    rows = []
    for name in graphs:
        n, deg = GRAPHS[name]
        g = make_sbm_graph(name, n, max(1, n // 128), deg, 1, seed=3)
        perm = np.random.default_rng(7).permutation(n)
        dsrc, ddst = torch.from_numpy(perm[g.src]).cuda(), torch.from_numpy(perm[g.dst]).cuda()
        adj = QGTC.pack_edges_tiled(dsrc, ddst, n, reorder=True)
        t = adj.T
        (deg_ms,) = timed_alternating(torch, [lambda: tiled._ext._tiled_degrees(adj.row_ptr, adj.kquad, adj.tiles, n)], reps)
        rec = {"graph": name, "order": "reordered", "n": n, "edges": int(g.src.size), "tiles": adj.n_tiles,
               "degrees_ms": deg_ms, "zero_out_degree": int((adj.degrees() == 0).sum()), "zero_in_degree": int((t.degrees() == 0).sum()),
               "agg": [], "saturation": []}
        print(f"{name:9s} T={adj.n_tiles} degrees + reciprocals, both directions {deg_ms[0]:.4f} ms [{deg_ms[1]:.4f}, {deg_ms[2]:.4f}]", flush=True)
        xr = np.random.default_rng(1)
        ones = torch.ones(n, dtype=torch.float32, device="cuda")
        for N in (16, 64, 256):
            for w in (1, 2):
                X = QGTC.val2bit(torch.from_numpy(xr.integers(0, 2 ** w, size=(n, N)).astype(np.float32)).cuda(), w, True, False)
                for a, direction in ((adj, "forward"), (t, "transposed")):
                    scale = a.mean_scale()
                    manual = lambda: QGTC.val2bit(QGTC.tiledMM2Int(a, X, N, w) * scale[:, None], w, False, False)  # noqa: E731
                    assert torch.equal(QGTC.tiledMM2Bit(a, X, N, w, w, scale), manual())
                    # a scale of ones gives the words of the unscaled call: the same data-dependent epilogue, plus the scale's cost
                    assert torch.equal(QGTC.tiledMM2Bit(a, X, N, w, w, ones), QGTC.tiledMM2Bit(a, X, N, w, w))
                    un, sc, one, man = timed_alternating(torch, [lambda: QGTC.tiledMM2Bit(a, X, N, w, w),
                                                                 lambda: QGTC.tiledMM2Bit(a, X, N, w, w, scale),
                                                                 lambda: QGTC.tiledMM2Bit(a, X, N, w, w, ones), manual], reps)
                    rec["agg"].append({"N": N, "w": w, "direction": direction, "unscaled_ms": un, "scaled_ms": sc, "scaled_ones_ms": one,
                                       "manual_ms": man, "scaled_over_unscaled": round(sc[0] / un[0], 3),
                                       "ones_over_unscaled": round(one[0] / un[0], 3), "manual_over_scaled": round(man[0] / sc[0], 3)})
                    print(f"{name:9s} N={N:<4d} w={w} {direction:10s} unscaled {un[0]:8.4f} [{un[1]:.4f}, {un[2]:.4f}]  mean scale {sc[0]:8.4f} "
                          f"[{sc[1]:.4f}, {sc[2]:.4f}] ({sc[0] / un[0]:.3f}x)  ones {one[0]:8.4f} ({one[0] / un[0]:.3f}x)  "
                          f"Int * scale, val2bit {man[0]:8.4f} ({man[0] / sc[0]:.2f}x)", flush=True)
                del X
        # what requant's clamp leaves of an in-neighbour aggregate: outputs at 2^b - 1, decoded from the kernels' own words
        for b in (2, 3, 4):
            N = 64
            X = QGTC.val2bit(torch.from_numpy(xr.integers(0, 2 ** b, size=(n, N)).astype(np.float32)).cuda(), b, True, False)
            v_sum = QGTC.bit2val(QGTC.tiledMM2Bit(t, X, N, b, b), b, n, N)
            v_mean = QGTC.bit2val(QGTC.tiledMM2Bit(t, X, N, b, b, t.mean_scale()), b, n, N)
            sat = {"bits": b, "sum_at_clamp": round(float((v_sum == 2 ** b - 1).float().mean()), 4),
                   "mean_at_clamp": round(float((v_mean == 2 ** b - 1).float().mean()), 4), "mean_distinct": int(torch.unique(v_mean).numel()),
                   "sum_distinct": int(torch.unique(v_sum).numel())}
            rec["saturation"].append(sat)
            print(f"{name:9s} in-neighbour aggregate at {b} bits, N = 64: at 2^b - 1 sum {sat['sum_at_clamp']:.4f} mean {sat['mean_at_clamp']:.4f}; "
                  f"distinct values sum {sat['sum_distinct']} mean {sat['mean_distinct']}", flush=True)
            del X, v_sum, v_mean
        rows.append(rec)
        del adj, t, dsrc, ddst
        torch.cuda.empty_cache()
    return rows


def float_leg(torch, QGTC, graphs, reps):
    from qgtc_ppopp22_amd.graph import make_sbm_graph

    rows = []
    for name in graphs:
        n, deg = GRAPHS[name]
        g = make_sbm_graph(name, n, max(1, n // 128), deg, 1, seed=3)
        perm = np.random.default_rng(7).permutation(n)
        dsrc, ddst = torch.from_numpy(perm[g.src]).cuda(), torch.from_numpy(perm[g.dst]).cuda()
        adj = QGTC.pack_edges_tiled(dsrc, ddst, n, reorder=True)
        t = adj.T
        cells = int(adj.degrees().sum())
        rec = {"graph": name, "order": "reordered", "n": n, "edges": int(g.src.size), "set_cells": cells, "tiles": adj.n_tiles,
               "max_out_degree": int(adj.degrees().max()), "max_in_degree": int(t.degrees().max()),
               "max_block_tiles": adj.max_block_tiles, "max_col_tiles": t.max_block_tiles, "agg": []}
        print(f"{name:9s} T={adj.n_tiles} set cells {cells} ({cells / max(1, adj.n_tiles):.1f} a tile)", flush=True)
        xr = np.random.default_rng(1)
        for N in (16, 64, 256):
            X = torch.from_numpy(xr.integers(0, 256, size=(n, N)).astype(np.float32)).cuda()
            bits = QGTC.val2bit(X, 8, True, False)
            floor_ms = (cells * N * 4 + n * N * 4 + 524 * adj.n_tiles) / HBM_BPS * 1e3
            for a, direction in ((adj, "forward"), (t, "transposed")):
                scale = a.mean_scale()
                for s, kind in ((None, "sum"), (scale, "mean")):   # integers below 2^24: the float and the bit route agree to the bit
                    assert torch.equal(QGTC.tiledMMFloat(a, X, s).view(torch.int32), QGTC.tiledMM2Int(a, bits, N, 8, s).view(torch.int32)), (N, direction, kind)
                fl, fs, bi, bv = timed_alternating(torch, [lambda: QGTC.tiledMMFloat(a, X), lambda: QGTC.tiledMMFloat(a, X, scale),
                                                           lambda: QGTC.tiledMM2Int(a, bits, N, 8),
                                                           lambda: QGTC.tiledMM2Int(a, QGTC.val2bit(X, 8, True, False), N, 8)], reps)
                rec["agg"].append({"N": N, "direction": direction, "float_ms": fl, "float_mean_ms": fs, "bit8_ms": bi, "bit8_with_val2bit_ms": bv,
                                   "float_over_bit8": round(fl[0] / bi[0], 3), "mean_over_sum": round(fs[0] / fl[0], 3),
                                   "floor_ms": round(floor_ms, 5), "floor_frac": round(floor_ms / fl[0], 4)})
                print(f"{name:9s} N={N:<4d} {direction:10s} float {fl[0]:8.4f} [{fl[1]:.4f}, {fl[2]:.4f}]  mean {fs[0]:8.4f} [{fs[1]:.4f}, {fs[2]:.4f}] "
                      f"({fs[0] / fl[0]:.3f}x)  8 planes {bi[0]:8.4f} [{bi[1]:.4f}, {bi[2]:.4f}] (float / planes {fl[0] / bi[0]:.3f})  "
                      f"with val2bit {bv[0]:8.4f}  floor {floor_ms:.4f} ms = {floor_ms / fl[0]:.3f} of the time", flush=True)
            del X, bits
        rows.append(rec)
        del adj, t, dsrc, ddst
        torch.cuda.empty_cache()
    return rows


def sym_leg(torch, QGTC, graphs, reps):
    from qgtc_ppopp22_amd.graph import make_sbm_graph

    rows = []
    for name in graphs:
        n, deg = GRAPHS[name]
        g = make_sbm_graph(name, n, max(1, n // 128), deg, 1, seed=3)
        perm = np.random.default_rng(7).permutation(n)
        dsrc, ddst = torch.from_numpy(perm[g.src]).cuda(), torch.from_numpy(perm[g.dst]).cuda()
        adj = QGTC.pack_edges_tiled(dsrc, ddst, n, reorder=True)
        t = adj.T
        cells = int(adj.degrees().sum())
        rec = {"graph": name, "order": "reordered", "n": n, "edges": int(g.src.size), "set_cells": cells, "tiles": adj.n_tiles, "agg": []}
        print(f"{name:9s} T={adj.n_tiles} set cells {cells} ({cells / max(1, adj.n_tiles):.1f} a tile)", flush=True)
        xr = np.random.default_rng(1)
        for N in (16, 64, 256):
            X = torch.from_numpy(xr.standard_normal((n, N)).astype(np.float32)).cuda()
            dY = torch.from_numpy(xr.standard_normal((n, N)).astype(np.float32)).cuda()
            Xg = X.clone().requires_grad_(True)
            for a, direction in ((adj, "forward"), (t, "transposed")):
                r, c = a.sym_scale(), a.T.sym_scale()
                manual = lambda: QGTC.tiledMMFloat(a, X * c[:, None], r)  # noqa: E731
                assert torch.equal(QGTC.tiledMMFloat(a, X, r, c).view(torch.int32), manual().view(torch.int32)), (N, direction)

                def both_ways():
                    return torch.autograd.grad(QGTC.tiledAggregate(a, Xg, r, c), Xg, dY)

                assert torch.equal(both_ways()[0].view(torch.int32), QGTC.tiledMMFloat(a.T, dY, c, r).view(torch.int32)), (N, direction)
                ta, tb, tc, td = timed_alternating(torch, [lambda: QGTC.tiledMMFloat(a, X, r), lambda: QGTC.tiledMMFloat(a, X, r, c),
                                                           manual, both_ways], reps)
                rec["agg"].append({"N": N, "direction": direction, "row_scale_ms": ta, "both_scales_ms": tb, "premultiplied_ms": tc,
                                   "forward_backward_ms": td, "both_over_row": round(tb[0] / ta[0], 3),
                                   "both_over_premultiplied": round(tb[0] / tc[0], 3), "fwd_bwd_over_both": round(td[0] / tb[0], 3)})
                print(f"{name:9s} N={N:<4d} {direction:10s} row scale {ta[0]:8.4f} [{ta[1]:.4f}, {ta[2]:.4f}]  both scales {tb[0]:8.4f} "
                      f"[{tb[1]:.4f}, {tb[2]:.4f}] ({tb[0] / ta[0]:.3f}x)  X * c, then row scale {tc[0]:8.4f} [{tc[1]:.4f}, {tc[2]:.4f}] "
                      f"(both / it {tb[0] / tc[0]:.3f})  forward + backward {td[0]:8.4f} [{td[1]:.4f}, {td[2]:.4f}]", flush=True)
            del X, dY, Xg
        rows.append(rec)
        del adj, t, dsrc, ddst
        torch.cuda.empty_cache()
    return rows


def max_leg(torch, QGTC, graphs, reps):
    from qgtc_ppopp22_amd import tiled
    from qgtc_ppopp22_amd.graph import make_sbm_graph

    rows = []
    for name in graphs:
        n, deg = GRAPHS[name]
        g = make_sbm_graph(name, n, max(1, n // 128), deg, 1, seed=3)
        perm = np.random.default_rng(7).permutation(n)
        dsrc, ddst = torch.from_numpy(perm[g.src]).cuda(), torch.from_numpy(perm[g.dst]).cuda()
        adj = QGTC.pack_edges_tiled(dsrc, ddst, n, reorder=True)
        t = adj.T
        cells = int(adj.degrees().sum())
        rec = {"graph": name, "order": "reordered", "n": n, "edges": int(g.src.size), "set_cells": cells, "tiles": adj.n_tiles, "agg": []}
        print(f"{name:9s} T={adj.n_tiles} set cells {cells} ({cells / max(1, adj.n_tiles):.1f} a tile)", flush=True)
        xr = np.random.default_rng(1)
        for N in (64, 256):
            X = torch.from_numpy(xr.standard_normal((n, N)).astype(np.float32)).cuda()
            dY = torch.from_numpy(xr.standard_normal((n, N)).astype(np.float32)).cuda()
            Xg = X.clone().requires_grad_(True)
            for a, direction in ((adj, "forward"), (t, "transposed")):
                out, arg = QGTC.tiledMMFloat(a, X, reduce="max", return_arg=True)
                has = arg >= 0                     # the value is the winner's own word; rows without neighbours give +0
                assert torch.equal(torch.where(has, X.gather(0, arg.clamp(min=0).long()), torch.zeros_like(X)).view(torch.int32),
                                   out.view(torch.int32)), (N, direction)
                assert torch.equal(has[:, 0], a.degrees() > 0)

                def both_ways():
                    return torch.autograd.grad(QGTC.tiledAggregate(a, Xg, reduce="max"), Xg, dY)

                assert torch.equal(both_ways()[0].view(torch.int32), tiled._tiled_select(a.T, dY, arg).view(torch.int32)), (N, direction)
                ts, tm, ta, tsel, tb = timed_alternating(torch, [lambda: QGTC.tiledMMFloat(a, X), lambda: QGTC.tiledMMFloat(a, X, reduce="max"),
                                                                 lambda: QGTC.tiledMMFloat(a, X, reduce="max", return_arg=True),
                                                                 lambda: tiled._tiled_select(a.T, dY, arg), both_ways], reps)
                rec["agg"].append({"N": N, "direction": direction, "sum_ms": ts, "max_ms": tm, "max_arg_ms": ta, "select_ms": tsel,
                                   "forward_backward_ms": tb, "max_over_sum": round(tm[0] / ts[0], 3),
                                   "max_arg_over_sum": round(ta[0] / ts[0], 3), "select_over_sum": round(tsel[0] / ts[0], 3),
                                   "fwd_bwd_over_max_arg": round(tb[0] / ta[0], 3)})
                print(f"{name:9s} N={N:<4d} {direction:10s} sum {ts[0]:8.4f} [{ts[1]:.4f}, {ts[2]:.4f}]  max {tm[0]:8.4f} [{tm[1]:.4f}, {tm[2]:.4f}] "
                      f"({tm[0] / ts[0]:.3f}x)  max + arg {ta[0]:8.4f} [{ta[1]:.4f}, {ta[2]:.4f}] ({ta[0] / ts[0]:.3f}x)  select on the other "
                      f"view {tsel[0]:8.4f} [{tsel[1]:.4f}, {tsel[2]:.4f}] ({tsel[0] / ts[0]:.3f}x)  forward + backward {tb[0]:8.4f} "
                      f"[{tb[1]:.4f}, {tb[2]:.4f}]", flush=True)
            del X, dY, Xg
        rows.append(rec)
        del adj, t, dsrc, ddst
        torch.cuda.empty_cache()
    return rows


def attn_leg(torch, QGTC, graphs, reps):
    from qgtc_ppopp22_amd.graph import make_sbm_graph

    rows = []
    for name in graphs:
        n, deg = GRAPHS[name]
        g = make_sbm_graph(name, n, max(1, n // 128), deg, 1, seed=3)
        perm = np.random.default_rng(7).permutation(n)
        dsrc, ddst = torch.from_numpy(perm[g.src]).cuda(), torch.from_numpy(perm[g.dst]).cuda()
        adj = QGTC.pack_edges_tiled(dsrc, ddst, n, reorder=True)
        t = adj.T
        cells = int(adj.degrees().sum())
        # the set cells as an edge list in the adjacency's numbering (multiplicity 2 is unset, as the packer quantises it)
        keys, counts = torch.unique(adj.rank.index_select(0, dsrc) * n + adj.rank.index_select(0, ddst), return_counts=True)
        keys = keys[counts != 2]
        e_row, e_col = keys // n, keys % n
        assert int(keys.numel()) == cells
        rec = {"graph": name, "order": "reordered", "n": n, "edges": int(g.src.size), "set_cells": cells, "tiles": adj.n_tiles, "agg": []}
        print(f"{name:9s} T={adj.n_tiles} set cells {cells} ({cells / max(1, adj.n_tiles):.1f} a tile)", flush=True)
        xr = np.random.default_rng(1)
        p = torch.from_numpy(xr.standard_normal(n).astype(np.float32)).cuda()
        q = torch.from_numpy(xr.standard_normal(n).astype(np.float32)).cuda()
        pg, qg = p.clone().requires_grad_(True), q.clone().requires_grad_(True)
        for N in (64, 256):
            X = torch.from_numpy(xr.standard_normal((n, N)).astype(np.float32)).cuda()
            dY = torch.from_numpy(xr.standard_normal((n, N)).astype(np.float32)).cuda()
            Xg = X.clone().requires_grad_(True)
            for a, direction in ((adj, "forward"), (t, "transposed")):
                r, c = a.sym_scale(), a.T.sym_scale()
                o, k = (e_col, e_row) if a.transposed else (e_row, e_col)

                def edge_list(Xe, pe, qe):
                    e = torch.nn.functional.leaky_relu(pe[o] + qe[k], 0.2)
                    mx = torch.full((n,), -float("inf"), device="cuda").scatter_reduce(0, o, e.detach(), "amax")
                    w = torch.exp(e - mx[o])
                    alpha = w / torch.zeros(n, device="cuda").index_add_(0, o, w)[o]
                    return torch.zeros(n, N, device="cuda").index_add_(0, o, alpha[:, None] * Xe[k])

                def att_both():
                    return torch.autograd.grad(QGTC.tiledAggregate(a, Xg, attn=(pg, qg)), (Xg, pg, qg), dY)

                def sym_both():
                    return torch.autograd.grad(QGTC.tiledAggregate(a, Xg, r, c), Xg, dY)

                def edge_both():
                    return torch.autograd.grad(edge_list(Xg, pg, qg), (Xg, pg, qg), dY)

                got, ref = QGTC.tiledMMFloat(a, X, attn=(p, q)), edge_list(X, p, q)
                assert torch.allclose(got, ref, rtol=1e-4, atol=1e-5), (N, direction, float((got - ref).abs().max()))
                for gk, ge in zip(att_both(), edge_both()):
                    assert torch.allclose(gk, ge, rtol=1e-3, atol=1e-4), (N, direction, float((gk - ge).abs().max()))
                ts, ta, tab, tsb, te, teb = timed_alternating(torch, [lambda: QGTC.tiledMMFloat(a, X, r, c),
                                                                      lambda: QGTC.tiledMMFloat(a, X, attn=(p, q)), att_both, sym_both,
                                                                      lambda: edge_list(X, p, q), edge_both], reps)
                rec["agg"].append({"N": N, "direction": direction, "sym_ms": ts, "attn_ms": ta, "attn_forward_backward_ms": tab,
                                   "sym_forward_backward_ms": tsb, "edge_list_ms": te, "edge_list_forward_backward_ms": teb,
                                   "attn_over_sym": round(ta[0] / ts[0], 3), "attn_fwd_bwd_over_sym_fwd_bwd": round(tab[0] / tsb[0], 3),
                                   "edge_list_over_attn": round(te[0] / ta[0], 3),
                                   "edge_list_fwd_bwd_over_attn_fwd_bwd": round(teb[0] / tab[0], 3)})
                print(f"{name:9s} N={N:<4d} {direction:10s} sym {ts[0]:8.4f} [{ts[1]:.4f}, {ts[2]:.4f}]  attn {ta[0]:8.4f} [{ta[1]:.4f}, {ta[2]:.4f}] "
                      f"({ta[0] / ts[0]:.3f}x)  attn fwd + bwd {tab[0]:8.4f} [{tab[1]:.4f}, {tab[2]:.4f}]  sym fwd + bwd {tsb[0]:8.4f} "
                      f"({tab[0] / tsb[0]:.3f}x)  edge list {te[0]:8.4f} [{te[1]:.4f}, {te[2]:.4f}] ({te[0] / ta[0]:.2f}x attn)  edge list fwd + bwd "
                      f"{teb[0]:8.4f} [{teb[1]:.4f}, {teb[2]:.4f}] ({teb[0] / tab[0]:.2f}x attn)", flush=True)
            del X, dY, Xg
        rows.append(rec)
        del adj, t, dsrc, ddst, keys, e_row, e_col
        torch.cuda.empty_cache()
    return rows


def drop_leg(torch, QGTC, graphs, reps):
    from qgtc_ppopp22_amd.graph import make_sbm_graph

    def mix32(x):   # include/qgtc.h, "Edge dropout", on int64 tensors kept below 2^32
        x = x ^ (x >> 16)
        x = (x * 0x7FEB352D) & 0xFFFFFFFF
        x = x ^ (x >> 15)
        x = (x * 0x846CA68B) & 0xFFFFFFFF
        return x ^ (x >> 16)

    def kept_cells(i, j, seed, rate):
        """bool tensor: the cells (i, j) the mask keeps, for the check before timing"""
        k0, k1 = seed & 0xFFFFFFFF, seed >> 32
        K = (int(mix32(torch.tensor(k0))) + k1) & 0xFFFFFFFF
        R, C = mix32(i ^ k0), (mix32(j ^ k1) + 0x9E3779B9) & 0xFFFFFFFF
        return mix32(((R ^ C) + K) & 0xFFFFFFFF) >= int(math.floor(rate * 4294967296.0))

    rows = []
    seed = 0x0123456789ABCDEF
    for name in graphs:
        n, deg = GRAPHS[name]
        g = make_sbm_graph(name, n, max(1, n // 128), deg, 1, seed=3)
        perm = np.random.default_rng(7).permutation(n)
        dsrc, ddst = torch.from_numpy(perm[g.src]).cuda(), torch.from_numpy(perm[g.dst]).cuda()
        adj = QGTC.pack_edges_tiled(dsrc, ddst, n, reorder=True)
        t = adj.T
        cells = int(adj.degrees().sum())
        # the set cells as an edge list in the adjacency's numbering (multiplicity 2 is unset, as the packer quantises it)
        keys, counts = torch.unique(adj.rank.index_select(0, dsrc) * n + adj.rank.index_select(0, ddst), return_counts=True)
        keys = keys[counts != 2]
        e_row, e_col = (keys // n).contiguous(), (keys % n).contiguous()
        assert int(keys.numel()) == cells
        rec = {"graph": name, "order": "reordered", "n": n, "edges": int(g.src.size), "set_cells": cells, "tiles": adj.n_tiles, "agg": []}
        print(f"{name:9s} T={adj.n_tiles} set cells {cells} ({cells / max(1, adj.n_tiles):.1f} a tile)", flush=True)
        kept = {}
        for rate in (0.1, 0.5):
            k = kept_cells(e_row, e_col, seed, rate)
            kept[rate] = QGTC.pack_edges_tiled(e_row[k], e_col[k], n, False)
            rec[f"kept_fraction_{rate}"] = round(float(k.float().mean()), 4)
        xr = np.random.default_rng(1)
        p = torch.from_numpy(xr.standard_normal(n).astype(np.float32)).cuda()
        q = torch.from_numpy(xr.standard_normal(n).astype(np.float32)).cuda()
        pg, qg = p.clone().requires_grad_(True), q.clone().requires_grad_(True)
        for N in (64, 256):
            X = torch.from_numpy(xr.standard_normal((n, N)).astype(np.float32)).cuda()
            dY = torch.from_numpy(xr.standard_normal((n, N)).astype(np.float32)).cuda()
            Xg = X.clone().requires_grad_(True)
            for a, direction in ((adj, "forward"), (t, "transposed")):
                for rate in (0.1, 0.5):
                    ka = kept[rate].T if a.transposed else kept[rate]
                    assert torch.equal(QGTC.tiledMMFloat(a, X, edge_drop=(rate, seed)).view(torch.int32),
                                       QGTC.tiledMMFloat(ka, X).view(torch.int32)), (N, direction, rate)

                def repack():
                    k = torch.rand(e_row.numel(), device="cuda") >= 0.1
                    sub = QGTC.pack_edges_tiled(e_row[k], e_col[k], n, False)
                    return QGTC.tiledMMFloat(sub.T if a.transposed else sub, X)

                ta, tb1, tb5, tc = timed_alternating(torch, [lambda: QGTC.tiledMMFloat(a, X),
                                                             lambda: QGTC.tiledMMFloat(a, X, edge_drop=(0.1, seed)),
                                                             lambda: QGTC.tiledMMFloat(a, X, edge_drop=(0.5, seed)), repack], reps)
                r, c = a.sym_scale(), a.T.sym_scale()

                def both(**kw):
                    return lambda: torch.autograd.grad(QGTC.tiledAggregate(a, Xg, **kw), [Xg] + ([pg, qg] if "attn" in kw else []), dY)

                drop = (0.1, seed)
                ds, dsm, dx, dxm, da, dam = timed_alternating(torch, [both(row_scale=r, src_scale=c), both(row_scale=r, src_scale=c, edge_drop=drop),
                                                                      both(reduce="max"), both(reduce="max", edge_drop=drop),
                                                                      both(attn=(pg, qg)), both(attn=(pg, qg), edge_drop=drop)], reps)
                rec["agg"].append({"N": N, "direction": direction, "plain_ms": ta, "masked_0.1_ms": tb1, "masked_0.5_ms": tb5,
                                   "filter_repack_plain_ms": tc, "masked_0.1_over_plain": round(tb1[0] / ta[0], 3),
                                   "masked_0.5_over_plain": round(tb5[0] / ta[0], 3), "masked_0.1_over_repack": round(tb1[0] / tc[0], 3),
                                   "sym_fwd_bwd_ms": ds, "sym_fwd_bwd_masked_ms": dsm, "max_fwd_bwd_ms": dx, "max_fwd_bwd_masked_ms": dxm,
                                   "attn_fwd_bwd_ms": da, "attn_fwd_bwd_masked_ms": dam, "sym_masked_over_plain": round(dsm[0] / ds[0], 3),
                                   "max_masked_over_plain": round(dxm[0] / dx[0], 3), "attn_masked_over_plain": round(dam[0] / da[0], 3)})
                print(f"{name:9s} N={N:<4d} {direction:10s} plain {ta[0]:8.4f} [{ta[1]:.4f}, {ta[2]:.4f}]  masked 0.1 {tb1[0]:8.4f} [{tb1[1]:.4f}, "
                      f"{tb1[2]:.4f}] ({tb1[0] / ta[0]:.3f}x)  masked 0.5 {tb5[0]:8.4f} [{tb5[1]:.4f}, {tb5[2]:.4f}] ({tb5[0] / ta[0]:.3f}x)  filter + "
                      f"pack + plain {tc[0]:8.4f} [{tc[1]:.4f}, {tc[2]:.4f}] (masked 0.1 / it {tb1[0] / tc[0]:.3f})  fwd + bwd plain / masked 0.1: "
                      f"sym {ds[0]:.4f} / {dsm[0]:.4f}  max {dx[0]:.4f} / {dxm[0]:.4f}  attn {da[0]:.4f} / {dam[0]:.4f}", flush=True)
            del X, dY, Xg
        rows.append(rec)
        del adj, t, dsrc, ddst, keys, e_row, e_col, kept
        torch.cuda.empty_cache()
    return rows


def nodes_leg(torch, QGTC, graphs, reps):
    from qgtc_ppopp22_amd.graph import make_sbm_graph
    from qgtc_ppopp22_amd.tiled import node_bitmap

    rows = []
    for name in graphs:
        n, deg = GRAPHS[name]
        g = make_sbm_graph(name, n, max(1, n // 128), deg, 1, seed=3)
        perm = np.random.default_rng(7).permutation(n)
        dsrc, ddst = torch.from_numpy(perm[g.src]).cuda(), torch.from_numpy(perm[g.dst]).cuda()
        adj = QGTC.pack_edges_tiled(dsrc, ddst, n, reorder=True)
        t = adj.T
        # the set cells as an edge list in the adjacency's numbering (multiplicity 2 is unset, as the packer quantises it)
        keys, counts = torch.unique(adj.rank.index_select(0, dsrc) * n + adj.rank.index_select(0, ddst), return_counts=True)
        keys = keys[counts != 2]
        e_row, e_col = (keys // n).contiguous(), (keys % n).contiguous()
        mr = np.random.default_rng(11)
        ids = np.arange(n)
        quads = (n + 127) // 128
        sets = {"contiguous_eighth": ids < n // 8,
                "community_eighth": np.isin(ids // 128, mr.permutation(quads)[: max(1, quads // 8)]),
                "random_eighth": mr.random(n) < 0.125,
                "rows_half": mr.random(n) < 0.5}
        ones = node_bitmap(torch.ones(n, dtype=torch.bool, device="cuda"), n)
        masks = {}
        for kind, f in sets.items():
            fl = torch.from_numpy(f).cuda()
            bm = node_bitmap(fl, n)
            masks[kind] = (fl, None, bm, None) if kind == "rows_half" else (fl, fl, bm, bm)
        rec = {"graph": name, "order": "reordered", "n": n, "edges": int(g.src.size), "set_cells": int(keys.numel()), "tiles": adj.n_tiles,
               "node_share": {k: round(float(f.mean()), 4) for k, f in sets.items()}, "agg": []}
        print(f"{name:9s} T={adj.n_tiles} set cells {int(keys.numel())}", flush=True)
        xr = np.random.default_rng(1)
        for N in (64, 256):
            X = torch.from_numpy(xr.standard_normal((n, N)).astype(np.float32)).cuda()
            dY = torch.from_numpy(xr.standard_normal((n, N)).astype(np.float32)).cuda()
            Xg = X.clone().requires_grad_(True)
            for a, direction in ((adj, "forward"), (t, "transposed")):
                e_out, e_nbr = (e_col, e_row) if a.transposed else (e_row, e_col)

                def induced(kind):
                    R, S = masks[kind][:2]
                    k = R[e_out] if S is None else R[e_out] & S[e_nbr]
                    sub = QGTC.pack_edges_tiled(e_row[k], e_col[k], n, False)
                    return sub.T if a.transposed else sub

                def masked(kind):
                    return lambda: QGTC.tiledMMFloat(a, X, row_mask=masks[kind][2], nbr_mask=masks[kind][3])

                out = {"N": N, "direction": direction}
                for kind in sets:
                    assert torch.equal(masked(kind)().view(torch.int32), QGTC.tiledMMFloat(induced(kind), X).view(torch.int32)), (N, direction, kind)
                    # one workgroup a k-quad on adj.T, a 32-row block on adj
                    words = masks[kind][2].view(-1, 4) if a.transposed else masks[kind][2][: (n + 31) // 32].view(-1, 1)
                    out[f"live_workgroups_{kind}"] = round(float((words != 0).any(dim=1).float().mean()), 4)
                assert torch.equal(QGTC.tiledMMFloat(a, X, row_mask=ones, nbr_mask=ones).view(torch.int32), QGTC.tiledMMFloat(a, X).view(torch.int32))
                kinds = list(sets)
                ta, *tm, to = timed_alternating(torch, [lambda: QGTC.tiledMMFloat(a, X)] + [masked(k) for k in kinds]
                                                + [lambda: QGTC.tiledMMFloat(a, X, row_mask=ones, nbr_mask=ones)], reps)
                tr = timed_alternating(torch, [(lambda k=k: QGTC.tiledMMFloat(induced(k), X)) for k in kinds], reps)
                r, c = a.sym_scale(), a.T.sym_scale()

                def both(**kw):
                    return lambda: torch.autograd.grad(QGTC.tiledAggregate(a, Xg, r, c, **kw), [Xg], dY)

                fb = timed_alternating(torch, [both()] + [both(row_mask=masks[k][2], nbr_mask=masks[k][3]) for k in kinds[:3]], reps)
                out.update({"plain_ms": ta, "all_ones_masked_ms": to, "all_ones_over_plain": round(to[0] / ta[0], 3), "sym_fwd_bwd_ms": fb[0]})
                line = f"{name:9s} N={N:<4d} {direction:10s} plain {ta[0]:.4f} [{ta[1]:.4f}, {ta[2]:.4f}]  all ones {to[0]:.4f} ({to[0] / ta[0]:.3f}x)"
                for i, k in enumerate(kinds):
                    out.update({f"masked_{k}_ms": tm[i], f"filter_repack_plain_{k}_ms": tr[i], f"masked_{k}_over_plain": round(tm[i][0] / ta[0], 3),
                                f"masked_{k}_over_repack": round(tm[i][0] / tr[i][0], 3)})
                    line += f"  {k} {tm[i][0]:.4f} [{tm[i][1]:.4f}, {tm[i][2]:.4f}] ({tm[i][0] / ta[0]:.3f}x plain, {tm[i][0] / tr[i][0]:.3f}x repack {tr[i][0]:.4f})"
                for i, k in enumerate(kinds[:3]):
                    out.update({f"sym_fwd_bwd_{k}_ms": fb[i + 1], f"sym_fwd_bwd_{k}_over_plain": round(fb[i + 1][0] / fb[0][0], 3)})
                    line += f"  fwd+bwd {k} {fb[i + 1][0]:.4f} / plain {fb[0][0]:.4f}"
                rec["agg"].append(out)
                print(line, flush=True)
            del X, dY, Xg
        rows.append(rec)
        del adj, t, dsrc, ddst, keys, e_row, e_col, masks
        torch.cuda.empty_cache()
    return rows


def bitnodes_leg(torch, QGTC, graphs, reps):
    from qgtc_ppopp22_amd.graph import make_sbm_graph
    from qgtc_ppopp22_amd.tiled import node_bitmap

    rows = []
    for name in graphs:
        n, deg = GRAPHS[name]
        g = make_sbm_graph(name, n, max(1, n // 128), deg, 1, seed=3)
        perm = np.random.default_rng(7).permutation(n)
        dsrc, ddst = torch.from_numpy(perm[g.src]).cuda(), torch.from_numpy(perm[g.dst]).cuda()
        adj = QGTC.pack_edges_tiled(dsrc, ddst, n, reorder=True)
        t = adj.T
        # the set cells as an edge list in the adjacency's numbering (multiplicity 2 is unset, as the packer quantises it)
        keys, counts = torch.unique(adj.rank.index_select(0, dsrc) * n + adj.rank.index_select(0, ddst), return_counts=True)
        keys = keys[counts != 2]
        e_row, e_col = (keys // n).contiguous(), (keys % n).contiguous()
        mr = np.random.default_rng(11)
        ids = np.arange(n)
        quads = (n + 127) // 128
        sets = {"contiguous_eighth": ids < n // 8,
                "community_eighth": np.isin(ids // 128, mr.permutation(quads)[: max(1, quads // 8)]),
                "random_eighth": mr.random(n) < 0.125,
                "rows_half": mr.random(n) < 0.5}
        ones = node_bitmap(torch.ones(n, dtype=torch.bool, device="cuda"), n)
        masks = {}
        for kind, f in sets.items():
            fl = torch.from_numpy(f).cuda()
            bm = node_bitmap(fl, n)
            masks[kind] = (fl, None, bm, None) if kind == "rows_half" else (fl, fl, bm, bm)
        rec = {"graph": name, "order": "reordered", "n": n, "edges": int(g.src.size), "set_cells": int(keys.numel()), "tiles": adj.n_tiles,
               "node_share": {k: round(float(f.mean()), 4) for k, f in sets.items()}, "agg": []}
        print(f"{name:9s} T={adj.n_tiles} set cells {int(keys.numel())}", flush=True)
        xr = np.random.default_rng(1)
        N = 64
        for w in (1, 2):
            X = QGTC.val2bit(torch.from_numpy(xr.integers(0, 2 ** w, size=(n, N)).astype(np.float32)).cuda(), w, True, False)
            for a, direction in ((adj, "forward"), (t, "transposed")):
                e_out, e_nbr = (e_col, e_row) if a.transposed else (e_row, e_col)

                def induced(kind):
                    R, S = masks[kind][:2]
                    k = R[e_out] if S is None else R[e_out] & S[e_nbr]
                    sub = QGTC.pack_edges_tiled(e_row[k], e_col[k], n, False)
                    return sub.T if a.transposed else sub

                def masked(kind):
                    return lambda: QGTC.tiledMM2Bit(a, X, N, w, w, row_mask=masks[kind][2], nbr_mask=masks[kind][3])

                out = {"N": N, "w": w, "direction": direction}
                for kind in sets:
                    assert torch.equal(masked(kind)(), QGTC.tiledMM2Bit(induced(kind), X, N, w, w)), (w, direction, kind)
                    # one workgroup a k-quad on adj.T, a 32-row block on adj
                    words = masks[kind][2].view(-1, 4) if a.transposed else masks[kind][2][: (n + 31) // 32].view(-1, 1)
                    out[f"live_workgroups_{kind}"] = round(float((words != 0).any(dim=1).float().mean()), 4)
                assert torch.equal(QGTC.tiledMM2Bit(a, X, N, w, w, row_mask=ones, nbr_mask=ones), QGTC.tiledMM2Bit(a, X, N, w, w))
                kinds = list(sets)
                ta, *tm, to = timed_alternating(torch, [lambda: QGTC.tiledMM2Bit(a, X, N, w, w)] + [masked(k) for k in kinds]
                                                + [lambda: QGTC.tiledMM2Bit(a, X, N, w, w, row_mask=ones, nbr_mask=ones)], reps)
                tr = timed_alternating(torch, [(lambda k=k: QGTC.tiledMM2Bit(induced(k), X, N, w, w)) for k in kinds], reps)
                out.update({"plain_ms": ta, "all_ones_masked_ms": to, "all_ones_over_plain": round(to[0] / ta[0], 3)})
                line = f"{name:9s} N={N:<4d} w={w} {direction:10s} plain {ta[0]:.4f} [{ta[1]:.4f}, {ta[2]:.4f}]  all ones {to[0]:.4f} ({to[0] / ta[0]:.3f}x)"
                for i, k in enumerate(kinds):
                    out.update({f"masked_{k}_ms": tm[i], f"filter_repack_plain_{k}_ms": tr[i], f"masked_{k}_over_plain": round(tm[i][0] / ta[0], 3),
                                f"masked_{k}_over_repack": round(tm[i][0] / tr[i][0], 3)})
                    line += f"  {k} {tm[i][0]:.4f} [{tm[i][1]:.4f}, {tm[i][2]:.4f}] ({tm[i][0] / ta[0]:.3f}x plain, {tm[i][0] / tr[i][0]:.3f}x repack {tr[i][0]:.4f})"
                rec["agg"].append(out)
                print(line, flush=True)
            del X
        rows.append(rec)
        del adj, t, dsrc, ddst, keys, e_row, e_col, masks
        torch.cuda.empty_cache()
    return rows


def affine_leg(torch, QGTC, graphs, reps):
    """Affine quantisation (qgtc_ppopp22_amd/affine.py) on the reordered graphs at N = 64: the range launch, the fused
    quantise + pack beside QGTC.val2bit at the same shape, the dequantising epilogue, affine.aggregate beside tiledMM2Int alone and beside
    tiledMMFloat, the layer's forward beside conv.GCNConv's, and the layer's relative error against the float layer. No pass mark."""
    from qgtc_ppopp22_amd import affine, conv
    from qgtc_ppopp22_amd.graph import make_sbm_graph

    rows = []
    N, dims = 64, (128, 64, 40)
    for name in graphs:
        n, deg = GRAPHS[name]
        g = make_sbm_graph(name, n, max(1, n // 128), deg, 1, seed=3)
        perm = np.random.default_rng(7).permutation(n)
        dsrc, ddst = torch.from_numpy(perm[g.src]).cuda(), torch.from_numpy(perm[g.dst]).cuda()
        adj = QGTC.pack_edges_tiled(dsrc, ddst, n, reorder=True)
        adj.T, adj.mean_scale()
        rec = {"graph": name, "order": "reordered", "n": n, "edges": int(g.src.size), "tiles": adj.n_tiles, "N": N, "dims": list(dims), "agg": []}
        xr = np.random.default_rng(1)
        X = torch.from_numpy(xr.normal(size=(n, N)).astype(np.float32)).cuda()
        Xpos = (X.abs() * 2.0).contiguous()      # what the parent's quantiser is meaningful on: values in [0, 2^b]
        x_bytes = n * N * 4
        qt, qc = timed_alternating(torch, [lambda: affine.qparams(X, 8), lambda: affine.qparams(X, 8, per_column=True)], reps)
        rec["qparams_ms"], rec["qparams_per_column_ms"] = qt, qc
        rec["qparams_GBps"] = round(x_bytes / qt[0] / 1e6, 1)
        print(f"{name:9s} n={n} N={N} qparams {qt[0]:.4f} ms ({rec['qparams_GBps']} GB/s of x)  per column {qc[0]:.4f} ms", flush=True)
        for bits in (2, 4, 8):
            qp = affine.qparams(X, bits)
            out = {"bits": bits}
            for cm, layout in ((False, "rows"), (True, "cols")):
                new, new_sums, old = timed_alternating(torch, [lambda: affine.val2bit_affine(X, bits, qp, cm, False),
                                                               lambda: affine.val2bit_affine(X, bits, qp, cm, True),
                                                               lambda: QGTC.val2bit(Xpos, bits, cm, False)], reps)
                out.update({f"val2bit_affine_{layout}_ms": new, f"val2bit_affine_{layout}_sums_ms": new_sums, f"val2bit_{layout}_ms": old,
                            f"affine_over_val2bit_{layout}": round(new[0] / old[0], 3), f"sums_launch_{layout}_ms": round(new_sums[0] - new[0], 4)})
                print(f"{name:9s} {bits} bits {layout}: val2bit_affine {new[0]:.4f} [{new[1]:.4f}, {new[2]:.4f}] ms, with sums {new_sums[0]:.4f}, "
                      f"val2bit {old[0]:.4f} [{old[1]:.4f}, {old[2]:.4f}] ms, ratio {new[0] / old[0]:.3f}", flush=True)
            bit_T, _ = affine.val2bit_affine(X, bits, qp, True, False)
            acc = QGTC.tiledMM2Int(adj, bit_T, N, bits)
            ident = affine._identity_qparams(X.device)
            degs = adj.degrees()
            want = affine.aggregate(adj, X, bits)
            exact = QGTC.tiledMMFloat(adj, X)
            out["aggregate_rel_error"] = round(float((want - exact).norm() / exact.norm()), 5)
            dq, agg, mm, fl = timed_alternating(torch, [lambda: affine.dequant(acc, n, ident, degs, qp, None),
                                                        lambda: affine.aggregate(adj, X, bits),
                                                        lambda: QGTC.tiledMM2Int(adj, bit_T, N, bits),
                                                        lambda: QGTC.tiledMMFloat(adj, X)], reps)
            out.update({"dequant_ms": dq, "aggregate_ms": agg, "tiledMM2Int_ms": mm, "tiledMMFloat_ms": fl,
                        "aggregate_over_mm2int": round(agg[0] / mm[0], 3), "aggregate_over_float": round(agg[0] / fl[0], 3)})
            print(f"{name:9s} {bits} bits: dequant {dq[0]:.4f} ms  aggregate {agg[0]:.4f} [{agg[1]:.4f}, {agg[2]:.4f}] ms  tiledMM2Int alone {mm[0]:.4f} ms  "
                  f"tiledMMFloat {fl[0]:.4f} ms  rel. error {out['aggregate_rel_error']}", flush=True)
            rec["agg"].append(out)
            del bit_T, acc, want, exact
        torch.manual_seed(0)
        ref = conv.GCNConv(*dims, norm="mean").cuda()
        with torch.no_grad():
            ref.W_in.mul_(dims[0] ** -0.5)
            ref.W_out.mul_(dims[1] ** -0.5)
        F = torch.from_numpy(xr.normal(size=(n, dims[0])).astype(np.float32)).cuda()
        with torch.no_grad():
            want = ref(adj, F)
        layer = {}
        for w_bit, act_bit in ((4, 4), (4, 8), (8, 8)):
            q = affine.GCNConv_Affine.from_float(ref, w_bit, act_bit)
            got = q(adj, F)
            err = float((got - want).norm() / want.norm())

            def float_forward():
                with torch.no_grad():
                    return ref(adj, F)

            tq, tf = timed_alternating(torch, [lambda: q(adj, F), float_forward], reps)
            layer[f"w{w_bit}a{act_bit}"] = {"forward_ms": tq, "float_forward_ms": tf, "over_float": round(tq[0] / tf[0], 3), "rel_error": round(err, 5)}
            print(f"{name:9s} layer {dims} w{w_bit} a{act_bit}: forward {tq[0]:.4f} [{tq[1]:.4f}, {tq[2]:.4f}] ms  conv.GCNConv {tf[0]:.4f} ms  "
                  f"({tq[0] / tf[0]:.2f}x)  rel. error against the float layer {err:.5f}", flush=True)
        rec["layer"] = layer
        rows.append(rec)
        del adj, dsrc, ddst, X, Xpos, F, want
        torch.cuda.empty_cache()
    return rows


def _separated(a, b):
    """whether timing a = (median, p10, p90) lies wholly below timing b: a's 90th percentile under b's 10th"""
    return a[2] < b[1]


def codes_leg(torch, QGTC, graphs, reps):
    """The byte-code route of affine quantisation (include/qgtc_codes.h) on the reordered graphs, Gaussian float32
    [n, 64] and [n, 256], adj and adj.T: affine.codes beside val2bit_affine in the cols layout at 8 bits, tiledMMCodes, aggregate on
    both routes at 2 / 4 / 8 bits in the same alternating rounds beside tiledMMFloat, and the layer at 128 / 64 / 40 dims with norm
    "mean" on both routes beside conv.GCNConv. Pass mark (4 and 8 bits only): the bytes route's 90th percentile lies under the planes
    route's 10th."""
    from qgtc_ppopp22_amd import affine, conv
    from qgtc_ppopp22_amd.graph import make_sbm_graph

    rows = []
    dims = (128, 64, 40)
    for name in graphs:
        n, deg = GRAPHS[name]
        g = make_sbm_graph(name, n, max(1, n // 128), deg, 1, seed=3)
        perm = np.random.default_rng(7).permutation(n)
        dsrc, ddst = torch.from_numpy(perm[g.src]).cuda(), torch.from_numpy(perm[g.dst]).cuda()
        adj = QGTC.pack_edges_tiled(dsrc, ddst, n, reorder=True)
        adj.T, adj.mean_scale()
        rec = {"graph": name, "order": "reordered", "n": n, "edges": int(g.src.size), "tiles": adj.n_tiles, "dims": list(dims), "agg": []}
        xr = np.random.default_rng(1)
        for N in (64, 256):
            X = torch.from_numpy(xr.normal(size=(n, N)).astype(np.float32)).cuda()
            qp = affine.qparams(X, 8)
            cd, pk = timed_alternating(torch, [lambda: affine.codes(X, 8, qp), lambda: affine.val2bit_affine(X, 8, qp, True, False)], reps)
            rec[f"codes_N{N}_ms"], rec[f"val2bit_affine_cols_N{N}_ms"] = cd, pk
            print(f"{name:9s} N={N}: codes {cd[0]:.4f} [{cd[1]:.4f}, {cd[2]:.4f}] ms  val2bit_affine cols 8 bits {pk[0]:.4f} [{pk[1]:.4f}, {pk[2]:.4f}] ms",
                  flush=True)
            Q = affine.codes(X, 8, qp)
            for view, a in (("adj", adj), ("adjT", adj.T)):
                assert torch.equal(affine.aggregate(a, X, 8, route="bytes").view(torch.int32), affine.aggregate(a, X, 8).view(torch.int32))
                mmc, fl = timed_alternating(torch, [lambda: affine.tiledMMCodes(a, Q), lambda: QGTC.tiledMMFloat(a, X)], reps)
                for bits in (2, 4, 8):
                    by, pl, f2 = timed_alternating(torch, [lambda: affine.aggregate(a, X, bits, route="bytes"),
                                                           lambda: affine.aggregate(a, X, bits, route="planes"),
                                                           lambda: QGTC.tiledMMFloat(a, X)], reps)
                    out = {"N": N, "view": view, "bits": bits, "bytes_ms": by, "planes_ms": pl, "tiledMMFloat_ms": f2,
                           "bytes_over_planes": round(by[0] / pl[0], 3), "bytes_over_float": round(by[0] / f2[0], 3),
                           "tiledMMCodes_ms": mmc, "tiledMMCodes_over_float": round(mmc[0] / fl[0], 3)}
                    if bits in (4, 8):
                        out["pass"] = _separated(by, pl)
                    rec["agg"].append(out)
                    print(f"{name:9s} N={N} {view:4s} {bits} bits: bytes {by[0]:.4f} [{by[1]:.4f}, {by[2]:.4f}] ms  planes {pl[0]:.4f} [{pl[1]:.4f}, {pl[2]:.4f}] ms  "
                          f"ratio {by[0] / pl[0]:.3f}  tiledMMFloat {f2[0]:.4f} ms  tiledMMCodes {mmc[0]:.4f} ms  pass {out.get('pass', '-')}", flush=True)
            del X, Q
        torch.manual_seed(0)
        ref = conv.GCNConv(*dims, norm="mean").cuda()
        with torch.no_grad():
            ref.W_in.mul_(dims[0] ** -0.5)
            ref.W_out.mul_(dims[1] ** -0.5)
        F = torch.from_numpy(xr.normal(size=(n, dims[0])).astype(np.float32)).cuda()
        layer = {}
        for w_bit, act_bit in ((4, 4), (4, 8)):
            qb = affine.GCNConv_Affine.from_float(ref, w_bit, act_bit, route="bytes")
            qpl = affine.GCNConv_Affine.from_float(ref, w_bit, act_bit)
            assert torch.equal(qb(adj, F).view(torch.int32), qpl(adj, F).view(torch.int32))

            def float_forward():
                with torch.no_grad():
                    return ref(adj, F)

            tb, tp, tf = timed_alternating(torch, [lambda: qb(adj, F), lambda: qpl(adj, F), float_forward], reps)
            layer[f"w{w_bit}a{act_bit}"] = {"bytes_ms": tb, "planes_ms": tp, "float_ms": tf, "bytes_over_planes": round(tb[0] / tp[0], 3),
                                            "bytes_over_float": round(tb[0] / tf[0], 3), "pass": _separated(tb, tp)}
            print(f"{name:9s} layer {dims} w{w_bit} a{act_bit}: bytes {tb[0]:.4f} [{tb[1]:.4f}, {tb[2]:.4f}] ms  planes {tp[0]:.4f} [{tp[1]:.4f}, {tp[2]:.4f}] ms  "
                  f"conv.GCNConv {tf[0]:.4f} ms", flush=True)
        rec["layer"] = layer
        rows.append(rec)
        del adj, dsrc, ddst, F
        torch.cuda.empty_cache()
    return rows


def edge_leg(torch, QGTC, graphs, reps):
    from qgtc_ppopp22_amd import tiled
    from qgtc_ppopp22_amd.graph import make_sbm_graph

    rows = []
    for name in graphs:
        n, deg = GRAPHS[name]
        g = make_sbm_graph(name, n, max(1, n // 128), deg, 1, seed=3)
        perm = np.random.default_rng(7).permutation(n)
        dsrc, ddst = torch.from_numpy(perm[g.src]).cuda(), torch.from_numpy(perm[g.dst]).cuda()
        adj = QGTC.pack_edges_tiled(dsrc, ddst, n, reorder=True)
        t = adj.T

        def index_and_slots():
            base = QGTC.TiledAdjacency(n, adj.row_ptr, adj.kquad, adj.tiles, adj.perm, adj.rank)
            return tiled.edge_slots(base, dsrc, ddst)

        rs, rd = adj.rank.index_select(0, dsrc), adj.rank.index_select(0, ddst)   # the packing alone, without the reordering
        pack_ms, index_ms = timed_alternating(torch, [lambda: QGTC.pack_edges_tiled(rs, rd, n, False), index_and_slots], max(3, reps // 3))
        e_row, e_col = (v.long() for v in tiled.edge_endpoints(adj))
        nnz = int(e_row.numel())
        rec = {"graph": name, "order": "reordered", "n": n, "edges": int(g.src.size), "set_cells": nnz, "tiles": adj.n_tiles,
               "pack_ms": pack_ms, "value_index_and_edge_slots_ms": index_ms,
               "extra_bytes_over_src_scale": 4 * nnz + 72 * adj.n_tiles - 4 * n, "agg": []}
        print(f"{name:9s} T={adj.n_tiles} set cells {nnz}; pack {pack_ms[0]:.4f} ms, value index + edge_slots {index_ms[0]:.4f} ms", flush=True)
        xr = np.random.default_rng(1)
        w = torch.from_numpy(xr.standard_normal(nnz).astype(np.float32)).cuda()
        c = torch.from_numpy(xr.standard_normal(n).astype(np.float32)).cuda()
        z = torch.zeros(n, device="cuda")
        wg = w.clone().requires_grad_(True)
        for N in (64, 256):
            X = torch.from_numpy(xr.standard_normal((n, N)).astype(np.float32)).cuda()
            dY = torch.from_numpy(xr.standard_normal((n, N)).astype(np.float32)).cuda()
            Xg = X.clone().requires_grad_(True)
            for a, direction in ((adj, "forward"), (t, "transposed")):
                o, k = (e_col, e_row) if a.transposed else (e_row, e_col)

                def edge_list(Xe, we):
                    return torch.zeros(n, N, device="cuda").index_add_(0, o, we[:, None] * Xe.index_select(0, k))

                def weighted_both():
                    return torch.autograd.grad(QGTC.tiledAggregate(a, Xg, edge_weight=wg), (Xg, wg), dY)

                def edge_both():
                    return torch.autograd.grad(edge_list(Xg, wg), (Xg, wg), dY)

                def grad_own():   # the attention's score gradient on this view: the same walk and dot, folded per row
                    return tiled._att(a, dY, att_mode="grad_own", att_own=z, att_nbr=z, negative_slope=0.2, shift=z, inv=c, other=X, D=z)

                got, ref = QGTC.tiledMMFloat(a, X, edge_weight=w), edge_list(X, w)
                assert torch.allclose(got, ref, rtol=1e-4, atol=1e-4), (N, direction, float((got - ref).abs().max()))
                for gk, ge in zip(weighted_both(), edge_both()):
                    assert torch.allclose(gk, ge, rtol=1e-3, atol=1e-3), (N, direction, float((gk - ge).abs().max()))
                tw, ts, tp, td, tg, twb, te, teb = timed_alternating(torch, [
                    lambda: QGTC.tiledMMFloat(a, X, edge_weight=w), lambda: QGTC.tiledMMFloat(a, X, src_scale=c), lambda: QGTC.tiledMMFloat(a, X),
                    lambda: tiled.tiledSDDMM(a, dY, X), grad_own, weighted_both, lambda: edge_list(X, w), edge_both], reps)
                plain_bytes = 512 * adj.n_tiles + 4 * nnz * N + 4 * n * N
                rec["agg"].append({"N": N, "direction": direction, "weighted_ms": tw, "src_scale_ms": ts, "plain_ms": tp, "sddmm_ms": td,
                                   "attn_grad_own_ms": tg, "weighted_forward_backward_ms": twb, "edge_list_ms": te,
                                   "edge_list_forward_backward_ms": teb, "weighted_over_src_scale": round(tw[0] / ts[0], 3),
                                   "byte_ratio": round((plain_bytes + 4 * nnz + 72 * adj.n_tiles) / (plain_bytes + 4 * nnz), 3),
                                   "sddmm_over_grad_own": round(td[0] / tg[0], 3), "edge_list_over_weighted": round(te[0] / tw[0], 3),
                                   "edge_list_fwd_bwd_over_weighted_fwd_bwd": round(teb[0] / twb[0], 3)})
                print(f"{name:9s} N={N:<4d} {direction:10s} weighted {tw[0]:8.4f} [{tw[1]:.4f}, {tw[2]:.4f}]  src_scale {ts[0]:8.4f} "
                      f"[{ts[1]:.4f}, {ts[2]:.4f}] ({tw[0] / ts[0]:.3f}x)  plain {tp[0]:8.4f}  sddmm {td[0]:8.4f} [{td[1]:.4f}, {td[2]:.4f}]  "
                      f"grad_own {tg[0]:8.4f} ({td[0] / tg[0]:.3f}x)  fwd + both grads {twb[0]:8.4f} [{twb[1]:.4f}, {twb[2]:.4f}]  edge list "
                      f"{te[0]:8.4f} ({te[0] / tw[0]:.2f}x)  edge list fwd + bwd {teb[0]:8.4f} ({teb[0] / twb[0]:.2f}x)", flush=True)
            del X, dY, Xg
        rows.append(rec)
        del adj, t, dsrc, ddst, e_row, e_col, w, wg
        torch.cuda.empty_cache()
    return rows


def esoftmax_leg(torch, QGTC, graphs, reps):
    from qgtc_ppopp22_amd import tiled
    from qgtc_ppopp22_amd.graph import make_sbm_graph

    rows = []
    for name in graphs:
        n, deg = GRAPHS[name]
        g = make_sbm_graph(name, n, max(1, n // 128), deg, 1, seed=3)
        perm = np.random.default_rng(7).permutation(n)
        dsrc, ddst = torch.from_numpy(perm[g.src]).cuda(), torch.from_numpy(perm[g.dst]).cuda()
        adj = QGTC.pack_edges_tiled(dsrc, ddst, n, reorder=True)
        t = adj.T
        e_row, e_col = (v.long() for v in tiled.edge_endpoints(adj))
        nnz = int(e_row.numel())
        rec = {"graph": name, "order": "reordered", "n": n, "edges": int(g.src.size), "set_cells": nnz, "tiles": adj.n_tiles,
               "max_block_tiles": adj.max_block_tiles, "max_col_tiles": t.max_block_tiles, "agg": []}
        print(f"{name:9s} T={adj.n_tiles} set cells {nnz}, longest row list {adj.max_block_tiles}, longest column list "
              f"{t.max_block_tiles}", flush=True)
        xr = np.random.default_rng(1)
        logits = torch.from_numpy((3 * xr.standard_normal(nnz)).astype(np.float32)).cuda()
        gl = torch.from_numpy(xr.standard_normal(nnz).astype(np.float32)).cuda()
        for N in (64, 256):   # d = N: the width of Q and K and of V
            scale = 1.0 / math.sqrt(N)
            Q, K, V, dY = (torch.from_numpy(xr.standard_normal((n, N)).astype(np.float32)).cuda() for _ in range(4))
            Qg, Kg, Vg = (x.clone().requires_grad_(True) for x in (Q, K, V))
            for a, direction in ((adj, "forward"), (t, "transposed")):
                o, k = (e_col, e_row) if a.transposed else (e_row, e_col)
                alpha = tiled.tiledEdgeSoftmax(a, logits)

                def edge_list(Qe, Ke, Ve):
                    s = (Qe.index_select(0, o) * Ke.index_select(0, k)).sum(dim=1) * scale
                    top = torch.full((n,), float("-inf"), device="cuda").scatter_reduce(0, o, s.detach(), "amax")
                    w = torch.exp(s - top.index_select(0, o))
                    den = torch.zeros(n, device="cuda").index_add_(0, o, w)
                    return torch.zeros(n, N, device="cuda").index_add_(0, o, (w / den.index_select(0, o))[:, None] * Ve.index_select(0, k))

                def att_both():
                    return torch.autograd.grad(tiled.tiledEdgeAttention(a, Qg, Kg, Vg), (Qg, Kg, Vg), dY)

                def edge_both():
                    return torch.autograd.grad(edge_list(Qg, Kg, Vg), (Qg, Kg, Vg), dY)

                got, ref = tiled.tiledEdgeAttention(a, Q, K, V), edge_list(Q, K, V)
                assert torch.allclose(got, ref, rtol=1e-3, atol=1e-4), (N, direction, float((got - ref).abs().max()))
                for gk, ge in zip(att_both(), edge_both()):
                    assert torch.allclose(gk, ge, rtol=1e-3, atol=1e-3), (N, direction, float((gk - ge).abs().max()))
                tsm, tsg, tsd, tw = timed_alternating(torch, [
                    lambda: tiled.tiledEdgeSoftmax(a, logits), lambda: tiled._edge_softmax_grad(a, alpha, gl),
                    lambda: tiled.tiledSDDMM(a, Q, K), lambda: QGTC.tiledMMFloat(a, V, edge_weight=alpha)], reps)
                taf, tab, tef, teb = timed_alternating(torch, [lambda: tiled.tiledEdgeAttention(a, Q, K, V), att_both,
                                                               lambda: edge_list(Q, K, V), edge_both], reps)
                rec["agg"].append({"N": N, "direction": direction, "softmax_ms": tsm, "softmax_grad_ms": tsg, "sddmm_ms": tsd,
                                   "weighted_ms": tw, "attention_forward_ms": taf, "attention_forward_backward_ms": tab,
                                   "edge_list_forward_ms": tef, "edge_list_forward_backward_ms": teb,
                                   "softmax_over_sddmm": round(tsm[0] / tsd[0], 3), "softmax_over_weighted": round(tsm[0] / tw[0], 3),
                                   "grad_over_sddmm": round(tsg[0] / tsd[0], 3), "grad_over_weighted": round(tsg[0] / tw[0], 3),
                                   "edge_list_over_attention_forward": round(tef[0] / taf[0], 3),
                                   "edge_list_over_attention_forward_backward": round(teb[0] / tab[0], 3)})
                print(f"{name:9s} N={N:<4d} {direction:10s} softmax {tsm[0]:8.4f} [{tsm[1]:.4f}, {tsm[2]:.4f}]  its gradient {tsg[0]:8.4f} "
                      f"[{tsg[1]:.4f}, {tsg[2]:.4f}]  sddmm {tsd[0]:8.4f} [{tsd[1]:.4f}, {tsd[2]:.4f}] ({tsm[0] / tsd[0]:.3f}x, "
                      f"{tsg[0] / tsd[0]:.3f}x)  weighted {tw[0]:8.4f} [{tw[1]:.4f}, {tw[2]:.4f}] ({tsm[0] / tw[0]:.3f}x, {tsg[0] / tw[0]:.3f}x)  "
                      f"attention fwd {taf[0]:8.4f} [{taf[1]:.4f}, {taf[2]:.4f}]  fwd + bwd {tab[0]:8.4f} [{tab[1]:.4f}, {tab[2]:.4f}]  "
                      f"edge list fwd {tef[0]:8.4f} ({tef[0] / taf[0]:.2f}x)  fwd + bwd {teb[0]:8.4f} ({teb[0] / tab[0]:.2f}x)", flush=True)
            del Q, K, V, dY, Qg, Kg, Vg
        rows.append(rec)
        del adj, t, dsrc, ddst, e_row, e_col, logits, gl
        torch.cuda.empty_cache()
    return rows


HEADS_SHAPES = ((8, 8), (4, 16), (8, 32), (4, 64))   # (heads, columns per head)


def heads_leg(torch, QGTC, graphs, reps):
    from qgtc_ppopp22_amd import tiled
    from qgtc_ppopp22_amd.graph import make_sbm_graph

    def bits(x):
        return x.contiguous().view(torch.int32)

    rows = []
    for name in graphs:
        n, deg = GRAPHS[name]
        g = make_sbm_graph(name, n, max(1, n // 128), deg, 1, seed=3)
        perm = np.random.default_rng(7).permutation(n)
        dsrc, ddst = torch.from_numpy(perm[g.src]).cuda(), torch.from_numpy(perm[g.dst]).cuda()
        adj = QGTC.pack_edges_tiled(dsrc, ddst, n, reorder=True)
        t = adj.T
        nnz = int(tiled.edge_endpoints(adj)[0].numel())
        rec = {"graph": name, "order": "reordered", "n": n, "edges": int(g.src.size), "set_cells": nnz, "tiles": adj.n_tiles, "agg": []}
        print(f"{name:9s} T={adj.n_tiles} set cells {nnz}", flush=True)
        xr = np.random.default_rng(1)
        for H, d in HEADS_SHAPES:
            Q, K, V, dY = (torch.from_numpy(xr.standard_normal((n, H * d)).astype(np.float32)).cuda() for _ in range(4))
            Qg, Kg, Vg = (x.clone().requires_grad_(True) for x in (Q, K, V))
            for a, direction in ((adj, "forward"), (t, "transposed")):
                def loop(Ql, Kl, Vl):   # the layer's forward before the heads shared a call
                    outs = []
                    for h in range(H):
                        c = slice(h * d, (h + 1) * d)
                        outs.append(tiled.tiledEdgeAttention(a, Ql[:, c].contiguous(), Kl[:, c].contiguous(), Vl[:, c].contiguous()))
                    return torch.cat(outs, dim=1)

                def one_both():
                    return torch.autograd.grad(tiled.tiledEdgeAttention(a, Qg, Kg, Vg, heads=H), (Qg, Kg, Vg), dY)

                def loop_both():
                    return torch.autograd.grad(loop(Qg, Kg, Vg), (Qg, Kg, Vg), dY)

                assert torch.equal(bits(tiled.tiledEdgeAttention(a, Q, K, V, heads=H)), bits(loop(Q, K, V))), (H, d, direction)
                for x, y in zip(one_both(), loop_both()):
                    assert torch.equal(bits(x), bits(y)), (H, d, direction)
                tof, tlf, tob, tlb = timed_alternating(torch, [lambda: tiled.tiledEdgeAttention(a, Q, K, V, heads=H), lambda: loop(Q, K, V),
                                                               one_both, loop_both], reps)
                ok_f, ok_b = tof[0] <= tlf[0] + (tlf[2] - tlf[1]), tob[0] <= tlb[0] + (tlb[2] - tlb[1])
                rec["agg"].append({"heads": H, "d": d, "direction": direction, "one_call_forward_ms": tof, "loop_forward_ms": tlf,
                                   "one_call_forward_backward_ms": tob, "loop_forward_backward_ms": tlb,
                                   "loop_over_one_call_forward": round(tlf[0] / tof[0], 3),
                                   "loop_over_one_call_forward_backward": round(tlb[0] / tob[0], 3),
                                   "forward_within_spread": bool(ok_f), "forward_backward_within_spread": bool(ok_b)})
                print(f"{name:9s} H={H} d={d:<3d} {direction:10s} forward: one call {tof[0]:8.4f} [{tof[1]:.4f}, {tof[2]:.4f}]  loop "
                      f"{tlf[0]:8.4f} [{tlf[1]:.4f}, {tlf[2]:.4f}] ({tlf[0] / tof[0]:.2f}x)  forward + backward: one call {tob[0]:8.4f} "
                      f"[{tob[1]:.4f}, {tob[2]:.4f}]  loop {tlb[0]:8.4f} [{tlb[1]:.4f}, {tlb[2]:.4f}] ({tlb[0] / tob[0]:.2f}x)"
                      f"{'' if ok_f and ok_b else '  SLOWER THAN THE LOOP'}", flush=True)
            del Q, K, V, dY, Qg, Kg, Vg
        rows.append(rec)
        del adj, t, dsrc, ddst
        torch.cuda.empty_cache()
    return rows


def gatheads_leg(torch, QGTC, graphs, reps):
    """The attention path (`attn=(p, q)`, the reducer of GAT) with scores [n, H] in ONE call against the loop over the heads of the same
    tree - per head a `.contiguous()` column slice and the single-head call, concatenated -, on the heads leg's graphs, shapes and
    rhythm: forward, and forward plus all three gradients, alternating in one loop. Outputs are checked bit for bit before timing."""
    from qgtc_ppopp22_amd.graph import make_sbm_graph

    def bits(x):
        return x.contiguous().view(torch.int32)

    rows = []
    for name in graphs:
        n, deg = GRAPHS[name]
        g = make_sbm_graph(name, n, max(1, n // 128), deg, 1, seed=3)
        perm = np.random.default_rng(7).permutation(n)
        dsrc, ddst = torch.from_numpy(perm[g.src]).cuda(), torch.from_numpy(perm[g.dst]).cuda()
        adj = QGTC.pack_edges_tiled(dsrc, ddst, n, reorder=True)
        t = adj.T
        rec = {"graph": name, "order": "reordered", "n": n, "edges": int(g.src.size), "tiles": adj.n_tiles, "agg": []}
        print(f"{name:9s} T={adj.n_tiles}", flush=True)
        xr = np.random.default_rng(1)
        for H, d in HEADS_SHAPES:
            X, dY = (torch.from_numpy(xr.standard_normal((n, H * d)).astype(np.float32)).cuda() for _ in range(2))
            P, Q = (torch.from_numpy(xr.uniform(-1, 1, (n, H)).astype(np.float32)).cuda() for _ in range(2))
            Xg, Pg, Qg = (x.clone().requires_grad_(True) for x in (X, P, Q))
            for a, direction in ((adj, "forward"), (t, "transposed")):
                def loop(Xl, Pl, Ql):   # the layer's aggregation before the heads shared a call
                    return torch.cat([QGTC.tiledAggregate(a, Xl[:, h * d:(h + 1) * d].contiguous(), attn=(Pl[:, h].contiguous(), Ql[:, h].contiguous()))
                                      for h in range(H)], dim=1)

                def one_both():
                    return torch.autograd.grad(QGTC.tiledAggregate(a, Xg, attn=(Pg, Qg)), (Xg, Pg, Qg), dY)

                def loop_both():
                    return torch.autograd.grad(loop(Xg, Pg, Qg), (Xg, Pg, Qg), dY)

                assert torch.equal(bits(QGTC.tiledAggregate(a, X, attn=(P, Q))), bits(loop(X, P, Q))), (H, d, direction)
                for x, y in zip(one_both(), loop_both()):
                    assert torch.equal(bits(x), bits(y)), (H, d, direction)
                tof, tlf, tob, tlb = timed_alternating(torch, [lambda: QGTC.tiledAggregate(a, X, attn=(P, Q)), lambda: loop(X, P, Q),
                                                               one_both, loop_both], reps)
                # the expectation: the one call beats the loop by more than the loop's own 10th-90th spread
                ok_f, ok_b = tof[0] < tlf[0] - (tlf[2] - tlf[1]), tob[0] < tlb[0] - (tlb[2] - tlb[1])
                rec["agg"].append({"heads": H, "d": d, "direction": direction, "one_call_forward_ms": tof, "loop_forward_ms": tlf,
                                   "one_call_forward_backward_ms": tob, "loop_forward_backward_ms": tlb,
                                   "loop_over_one_call_forward": round(tlf[0] / tof[0], 3),
                                   "loop_over_one_call_forward_backward": round(tlb[0] / tob[0], 3),
                                   "forward_beats_the_loop_by_more_than_its_spread": bool(ok_f),
                                   "forward_backward_beats_the_loop_by_more_than_its_spread": bool(ok_b)})
                print(f"{name:9s} H={H} d={d:<3d} {direction:10s} forward: one call {tof[0]:8.4f} [{tof[1]:.4f}, {tof[2]:.4f}]  loop "
                      f"{tlf[0]:8.4f} [{tlf[1]:.4f}, {tlf[2]:.4f}] ({tlf[0] / tof[0]:.2f}x)  forward + backward: one call {tob[0]:8.4f} "
                      f"[{tob[1]:.4f}, {tob[2]:.4f}]  loop {tlb[0]:8.4f} [{tlb[1]:.4f}, {tlb[2]:.4f}] ({tlb[0] / tob[0]:.2f}x)"
                      f"{'' if ok_f and ok_b else '  NOT AHEAD OF THE LOOP BY ITS SPREAD'}", flush=True)
            del X, dY, P, Q, Xg, Pg, Qg
        rows.append(rec)
        del adj, t, dsrc, ddst
        torch.cuda.empty_cache()
    return rows


def gatv2_leg(torch, QGTC, graphs, reps):
    """The additive edge score of GATv2 (tiled.tiledEdgeAdditiveScores / tiledEdgeAdditiveAttention) on the heads leg's
    graphs and shapes, both directions. Three alternating loops: (a) the score launch against the tiledSDDMM(heads=H) launch of the same
    shape - the same walk and traffic, so the difference is the extra VALU work; (b) each gradient launch (d_own + P on the view, d_nbr
    alone on the other view) against the edge_weight weighted launch of the same shape and view; (c) the attention's forward and
    forward plus all four gradients against the edge-list route in torch (edge_endpoints, index_select, leaky_relu, a scatter softmax,
    index_add_, with its autograd backward, which is not bit-reproducible). The attention is checked against the edge-list route
    before timing. A cell slower than the edge-list route is printed as such."""
    from qgtc_ppopp22_amd import tiled
    from qgtc_ppopp22_amd.graph import make_sbm_graph

    slope = 0.2
    rows = []
    for name in graphs:
        n, deg = GRAPHS[name]
        g = make_sbm_graph(name, n, max(1, n // 128), deg, 1, seed=3)
        perm = np.random.default_rng(7).permutation(n)
        dsrc, ddst = torch.from_numpy(perm[g.src]).cuda(), torch.from_numpy(perm[g.dst]).cuda()
        adj = QGTC.pack_edges_tiled(dsrc, ddst, n, reorder=True)
        t = adj.T
        e_row, e_col = (v.long() for v in tiled.edge_endpoints(adj))
        nnz = int(e_row.numel())
        rec = {"graph": name, "order": "reordered", "n": n, "edges": int(g.src.size), "set_cells": nnz, "tiles": adj.n_tiles, "agg": []}
        print(f"{name:9s} T={adj.n_tiles} set cells {nnz}", flush=True)
        xr = np.random.default_rng(1)
        for H, d in HEADS_SHAPES:
            own, nbr, dY = (torch.from_numpy(xr.standard_normal((n, H * d)).astype(np.float32)).cuda() for _ in range(3))
            att = torch.from_numpy((xr.standard_normal((H, d)) / math.sqrt(d)).astype(np.float32)).cuda()
            gs = torch.from_numpy(xr.standard_normal((nnz, H)).astype(np.float32)).cuda()
            leaves = [x.clone().requires_grad_(True) for x in (own, nbr, att)]
            for a, direction in ((adj, "forward"), (t, "transposed")):
                o, k = (e_col, e_row) if a.transposed else (e_row, e_col)

                def edge_list(own_e, nbr_e, att_e):
                    u = torch.nn.functional.leaky_relu(own_e.index_select(0, o) + nbr_e.index_select(0, k), slope)
                    s = (u.view(nnz, H, d) * att_e).sum(dim=2)                                   # [nnz, H]
                    top = torch.full((n, H), float("-inf"), device="cuda").scatter_reduce(0, o[:, None].expand(nnz, H), s.detach(), "amax")
                    w = torch.exp(s - top.index_select(0, o))
                    den = torch.zeros(n, H, device="cuda").index_add_(0, o, w)
                    alpha = w / den.index_select(0, o)
                    msg = alpha[:, :, None] * nbr_e.index_select(0, k).view(nnz, H, d)
                    return torch.zeros(n, H * d, device="cuda").index_add_(0, o, msg.view(nnz, H * d))

                def one(own_e, nbr_e, att_e):   # the layer's aggregation: V is the neighbour operand
                    return tiled.tiledEdgeAdditiveAttention(a, own_e, nbr_e, nbr_e, att_e, slope, heads=H)

                def one_both():
                    return torch.autograd.grad(one(*leaves), leaves, dY)

                def edge_both():
                    return torch.autograd.grad(edge_list(*leaves), leaves, dY)

                got, ref = one(own, nbr, att), edge_list(own, nbr, att)
                assert torch.allclose(got, ref, rtol=1e-3, atol=1e-4), (H, d, direction, float((got - ref).abs().max()))
                for gk, ge in zip(one_both(), edge_both()):
                    assert torch.allclose(gk, ge, rtol=1e-3, atol=2e-3), (H, d, direction, float((gk - ge).abs().max()))
                tsc, tsd = timed_alternating(torch, [lambda: tiled.tiledEdgeAdditiveScores(a, own, nbr, att, slope, heads=H),
                                                     lambda: tiled.tiledSDDMM(a, own, nbr, heads=H)], reps)
                tg2, tg1, tw, twt = timed_alternating(torch, [
                    lambda: tiled._addscore_grad(a, own, nbr, att, slope, gs, H, True, True),
                    lambda: tiled._addscore_grad(a.T, nbr, own, att, slope, gs, H, True, False),
                    lambda: QGTC.tiledMMFloat(a, nbr, edge_weight=gs), lambda: QGTC.tiledMMFloat(a.T, own, edge_weight=gs)], reps)
                tof, tob, tef, teb = timed_alternating(torch, [lambda: one(own, nbr, att), one_both, lambda: edge_list(own, nbr, att), edge_both],
                                                       reps)
                slower = [what for what, mine, theirs in (("forward", tof, tef), ("forward + backward", tob, teb)) if mine[0] > theirs[0]]
                rec["agg"].append({"heads": H, "d": d, "direction": direction, "score_ms": tsc, "sddmm_ms": tsd,
                                   "grad_own_P_ms": tg2, "grad_nbr_other_view_ms": tg1, "weighted_ms": tw, "weighted_other_view_ms": twt,
                                   "attention_forward_ms": tof, "attention_forward_backward_ms": tob, "edge_list_forward_ms": tef,
                                   "edge_list_forward_backward_ms": teb, "score_over_sddmm": round(tsc[0] / tsd[0], 3),
                                   "grad_own_P_over_weighted": round(tg2[0] / tw[0], 3),
                                   "grad_nbr_over_weighted_other_view": round(tg1[0] / twt[0], 3),
                                   "edge_list_over_attention_forward": round(tef[0] / tof[0], 3),
                                   "edge_list_over_attention_forward_backward": round(teb[0] / tob[0], 3),
                                   "slower_than_the_edge_list": slower})
                print(f"{name:9s} H={H} d={d:<3d} {direction:10s} score {tsc[0]:8.4f} [{tsc[1]:.4f}, {tsc[2]:.4f}]  sddmm {tsd[0]:8.4f} "
                      f"[{tsd[1]:.4f}, {tsd[2]:.4f}] ({tsc[0] / tsd[0]:.3f}x)  d_own + P {tg2[0]:8.4f} [{tg2[1]:.4f}, {tg2[2]:.4f}]  weighted "
                      f"{tw[0]:8.4f} [{tw[1]:.4f}, {tw[2]:.4f}] ({tg2[0] / tw[0]:.3f}x)  d_nbr {tg1[0]:8.4f} [{tg1[1]:.4f}, {tg1[2]:.4f}]  "
                      f"weighted, other view {twt[0]:8.4f} [{twt[1]:.4f}, {twt[2]:.4f}] ({tg1[0] / twt[0]:.3f}x)  attention fwd {tof[0]:8.4f} "
                      f"[{tof[1]:.4f}, {tof[2]:.4f}]  fwd + bwd {tob[0]:8.4f} [{tob[1]:.4f}, {tob[2]:.4f}]  edge list fwd {tef[0]:8.4f} "
                      f"({tef[0] / tof[0]:.2f}x)  fwd + bwd {teb[0]:8.4f} ({teb[0] / tob[0]:.2f}x)"
                      f"{'  SLOWER THAN THE EDGE LIST: ' + ', '.join(slower) if slower else ''}", flush=True)
            del own, nbr, dY, att, gs, leaves
        rows.append(rec)
        del adj, t, dsrc, ddst, e_row, e_col
        torch.cuda.empty_cache()
    return rows


def fanout_leg(torch, QGTC, graphs, reps):
    from qgtc_ppopp22_amd import fanout, tiled
    from qgtc_ppopp22_amd.graph import make_sbm_graph

    rows = []
    seed = 0x0123456789ABCDEF
    for name in graphs:
        n, deg = GRAPHS[name]
        g = make_sbm_graph(name, n, max(1, n // 128), deg, 1, seed=3)
        perm = np.random.default_rng(7).permutation(n)
        dsrc, ddst = torch.from_numpy(perm[g.src]).cuda(), torch.from_numpy(perm[g.dst]).cuda()
        adj = QGTC.pack_edges_tiled(dsrc, ddst, n, reorder=True)
        t = adj.T
        e_row, e_col = (e.long() for e in tiled.edge_endpoints(adj))   # the set cells in slot order, the adjacency's numbering
        cells = int(e_row.numel())
        rec = {"graph": name, "order": "reordered", "n": n, "edges": int(g.src.size), "set_cells": cells, "tiles": adj.n_tiles,
               "max_out_degree": int(adj.degrees().max()), "max_in_degree": int(t.degrees().max()), "max_block_tiles": adj.max_block_tiles,
               "max_col_tiles": t.max_block_tiles, "agg": []}
        print(f"{name:9s} T={adj.n_tiles} set cells {cells}  largest degree out {rec['max_out_degree']} in {rec['max_in_degree']}", flush=True)
        xr = np.random.default_rng(1)

        def topk_repack(a, k):
            """today's route: fresh keys, the k largest per node of the view's axis by one sort, a second adjacency, the plain launch"""
            own = (e_col if a.transposed else e_row).to(torch.float64)
            order = torch.argsort(own + torch.rand(cells, device="cuda", dtype=torch.float64))
            first = torch.searchsorted(own[order], own[order])   # the first position of the node's run
            keep = order[torch.arange(cells, device="cuda") - first < k]
            return QGTC.pack_edges_tiled(e_row[keep], e_col[keep], n, False)

        for N in (64, 256):
            X = torch.from_numpy(xr.standard_normal((n, N)).astype(np.float32)).cuda()
            dY = torch.from_numpy(xr.standard_normal((n, N)).astype(np.float32)).cuda()
            Xg = X.clone().requires_grad_(True)
            for a, direction in ((adj, "forward"), (t, "transposed")):
                for k in (5, 10, 25):
                    own, other = fanout.sample_fanout(a, k, seed), fanout.sample_fanout(a.T, k, seed)
                    kept = int(a.degrees().clamp(max=k).sum())
                    got = QGTC.tiledMMFloat(a, torch.ones((n, 1), device="cuda"), fanout=own)
                    assert int(got.sum()) == kept and torch.equal(got.view(-1).to(torch.int32), a.degrees().clamp(max=k)), (N, direction, k)
                    rate = min(max(1.0 - kept / max(1, cells), 0.0), 1.0 - 2.0 ** -32)
                    scale = tiled._inv_degree(a.degrees().clamp(max=k))

                    def repack():
                        sub = topk_repack(a, k)
                        return QGTC.tiledMMFloat(sub.T if a.transposed else sub, X)

                    def both(**kw):
                        return lambda: torch.autograd.grad(QGTC.tiledAggregate(a, Xg, **kw), [Xg], dY)

                    def repack_both():
                        sub = topk_repack(a, k)
                        return torch.autograd.grad(QGTC.tiledAggregate(sub.T if a.transposed else sub, Xg, scale), [Xg], dY)

                    tsel, town, tnbr, tplain, tdrop, tpair = timed_alternating(torch, [
                        lambda: fanout.sample_fanout(a, k, seed), lambda: QGTC.tiledMMFloat(a, X, fanout=own),
                        lambda: QGTC.tiledMMFloat(a, X, fanout=other), lambda: QGTC.tiledMMFloat(a, X),
                        lambda: QGTC.tiledMMFloat(a, X, edge_drop=(rate, seed)), lambda: QGTC.tiledMMFloat(a, X, fanout=(k, seed))], reps)
                    (trepack,) = timed_alternating(torch, [repack], max(3, reps // 2))
                    bf, bp, bd = timed_alternating(torch, [both(row_scale=scale, fanout=(k, seed)), both(row_scale=scale),
                                                           both(row_scale=scale, edge_drop=(rate, seed))], reps)
                    (br,) = timed_alternating(torch, [repack_both], max(3, reps // 2))
                    rec["agg"].append({"N": N, "direction": direction, "k": k, "kept_cells": kept, "kept_fraction": round(kept / max(1, cells), 4),
                                       "select_ms": tsel, "own_ms": town, "nbr_ms": tnbr, "plain_ms": tplain, "edge_drop_same_edges_ms": tdrop,
                                       "select_plus_own_ms": tpair, "topk_repack_plain_ms": trepack, "fwd_bwd_fanout_ms": bf,
                                       "fwd_bwd_plain_ms": bp, "fwd_bwd_edge_drop_ms": bd, "fwd_bwd_topk_repack_ms": br,
                                       "repack_over_fanout": round(trepack[0] / tpair[0], 3), "own_over_plain": round(town[0] / tplain[0], 3),
                                       "nbr_over_own": round(tnbr[0] / town[0], 3), "own_over_edge_drop": round(town[0] / tdrop[0], 3),
                                       "fwd_bwd_repack_over_fanout": round(br[0] / bf[0], 3), "fwd_bwd_fanout_over_plain": round(bf[0] / bp[0], 3)})
                    print(f"{name:9s} N={N:<4d} {direction:10s} k={k:<3d} kept {kept / max(1, cells):.3f}  select {tsel[0]:8.4f}  own {town[0]:8.4f}  "
                          f"nbr {tnbr[0]:8.4f}  plain {tplain[0]:8.4f}  edge_drop {tdrop[0]:8.4f}  select+own {tpair[0]:8.4f}  top-k + pack + plain "
                          f"{trepack[0]:8.4f} ({trepack[0] / tpair[0]:.2f}x)  fwd+bwd fanout {bf[0]:8.4f} plain {bp[0]:8.4f} edge_drop {bd[0]:8.4f} "
                          f"top-k route {br[0]:8.4f} ({br[0] / bf[0]:.2f}x)", flush=True)
                    del own, other
            del X, dY, Xg
        rows.append(rec)
        del adj, t, dsrc, ddst, e_row, e_col
        torch.cuda.empty_cache()
    return rows


def blocks_leg(torch, QGTC, graphs, reps):
    from qgtc_ppopp22_amd import fanout, tiled
    from qgtc_ppopp22_amd.graph import make_sbm_graph

    rows = []
    seed, fanouts, members = 0x0123456789ABCDEF, (25, 10), 1024
    for name in graphs:
        n, deg = GRAPHS[name]
        g = make_sbm_graph(name, n, max(1, n // 128), deg, 1, seed=3)
        perm = np.random.default_rng(7).permutation(n)
        dsrc, ddst = torch.from_numpy(perm[g.src]).cuda(), torch.from_numpy(perm[g.dst]).cuda()
        adj = QGTC.pack_edges_tiled(dsrc, ddst, n, reorder=True)
        adj.T
        e_row, e_col = (e.long() for e in tiled.edge_endpoints(adj))   # the set cells in slot order, the adjacency's numbering
        cells = int(e_row.numel())
        flags = torch.zeros(n, dtype=torch.bool, device="cuda")
        flags[torch.from_numpy(np.random.default_rng(11).permutation(n)[:members]).cuda()] = True
        seeds = tiled.node_bitmap(flags, n)
        blocks = fanout.sample_blocks(adj, seeds, fanouts, seed)
        sizes = [int(flags.sum())] + [_popcount(torch, b.inputs) for b in blocks[::-1]]
        kept = [int(b.sample.counts.sum()) for b in blocks[::-1]]
        rec = {"graph": name, "order": "reordered", "n": n, "set_cells": cells, "tiles": adj.n_tiles, "seeds": members, "fanouts": list(fanouts),
               "rows_per_hop": sizes, "kept_cells_per_hop": kept, "agg": []}
        print(f"{name:9s} T={adj.n_tiles} set cells {cells}  rows per hop (seeds first) {sizes}  kept cells per hop {kept}", flush=True)
        xr = np.random.default_rng(1)

        def today(X):
            """per hop, last layer first: the edges of the row set, the k largest fresh keys per row by one sort, a second adjacency, the
            plain mean launch, the next row set"""
            rows_now, outs = flags, []
            for k in fanouts[::-1]:
                sel = rows_now[e_row]
                er, ec = e_row[sel], e_col[sel]
                own = er.to(torch.float64)
                order = torch.argsort(own + torch.rand(er.numel(), device="cuda", dtype=torch.float64))
                first = torch.searchsorted(own[order], own[order])
                keep = order[torch.arange(er.numel(), device="cuda") - first < k]
                sub = QGTC.pack_edges_tiled(er[keep], ec[keep], n, False)
                outs.append(QGTC.tiledMMFloat(sub, X, sub.mean_scale()))
                rows_now = rows_now.clone()
                rows_now[ec[keep]] = True
            return outs

        def new(X):
            return [QGTC.tiledMMFloat(adj, X, b.sample.mean_scale(), fanout=b.sample) for b in fanout.sample_blocks(adj, seeds, fanouts, seed)]

        for N in (64, 256):
            X = torch.from_numpy(xr.standard_normal((n, N)).astype(np.float32)).cuda()
            tnew, tbuild = timed_alternating(torch, [lambda: new(X), lambda: fanout.sample_blocks(adj, seeds, fanouts, seed)], reps)
            (ttoday,) = timed_alternating(torch, [lambda: today(X)], max(3, reps // 2))
            rec["agg"].append({"what": "batch", "N": N, "blocks_plus_aggregates_ms": tnew, "blocks_alone_ms": tbuild, "today_ms": ttoday,
                               "today_over_new": round(ttoday[0] / tnew[0], 3)})
            print(f"{name:9s} (a) N={N:<4d} blocks + 2 aggregates {tnew[0]:8.4f} [{tnew[1]:.4f}, {tnew[2]:.4f}]  blocks alone {tbuild[0]:8.4f}  "
                  f"today's route {ttoday[0]:8.4f} [{ttoday[1]:.4f}, {ttoday[2]:.4f}] ({ttoday[0] / tnew[0]:.2f}x)", flush=True)
            del X
        ones = torch.ones((n, 1), device="cuda")
        for hop, b in zip(("seeds", "inputs"), blocks[::-1]):
            s, k = b.sample, b.sample.k

            def three():
                return tiled.node_bitmap(QGTC.tiledMMFloat(adj.T, ones, fanout=s).view(n) > 0, n) | s.row_mask

            assert torch.equal(three(), fanout.frontier(s, include=True)), hop
            tfr, t3 = timed_alternating(torch, [lambda: fanout.frontier(s, include=True), three], reps)
            tmask, tall = timed_alternating(torch, [lambda: fanout.sample_fanout(adj, k, seed, row_mask=s.row_mask),
                                                    lambda: fanout.sample_fanout(adj, k, seed)], reps)
            rec["agg"].append({"what": "hop", "hop": hop, "k": k, "frontier_ms": tfr, "three_launches_ms": t3, "masked_selection_ms": tmask,
                               "unmasked_selection_ms": tall, "three_over_frontier": round(t3[0] / tfr[0], 3),
                               "masked_over_unmasked": round(tmask[0] / tall[0], 3)})
            print(f"{name:9s} (b) {hop:6s} k={k:<3d} frontier {tfr[0]:8.4f} [{tfr[1]:.4f}, {tfr[2]:.4f}]  three launches {t3[0]:8.4f} "
                  f"[{t3[1]:.4f}, {t3[2]:.4f}] ({t3[0] / tfr[0]:.2f}x)   (c) masked selection {tmask[0]:8.4f} [{tmask[1]:.4f}, {tmask[2]:.4f}]  "
                  f"unmasked {tall[0]:8.4f} [{tall[1]:.4f}, {tall[2]:.4f}] ({tmask[0] / tall[0]:.2f}x)", flush=True)
        rows.append(rec)
        del adj, dsrc, ddst, e_row, e_col, blocks
        torch.cuda.empty_cache()
    return rows


def _popcount(torch, bitmap):
    """the set bits of an int32 bitmap"""
    b = bitmap.to(torch.int64) & 0xFFFFFFFF
    return int(sum(((b >> i) & 1).sum() for i in range(32)))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="arxiv,reddit,products")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", default=None)
    ap.add_argument("--leg", default="orders", choices=("orders", "transposed", "scaled", "float", "sym", "max", "attn", "drop", "nodes", "edge", "esoftmax", "heads", "gatheads", "gatv2", "fanout", "blocks", "bitnodes", "affine", "codes"))
    args = ap.parse_args()

    import torch

    import QGTC
    from qgtc_ppopp22_amd.graph import make_sbm_graph

    if args.leg in ("transposed", "scaled", "float", "sym", "max", "attn", "drop", "nodes", "edge", "esoftmax", "heads", "gatheads", "gatv2", "fanout", "blocks", "bitnodes", "affine", "codes"):
        leg = {"transposed": transposed_leg, "scaled": scaled_leg, "float": float_leg, "sym": sym_leg, "max": max_leg, "attn": attn_leg,
               "drop": drop_leg, "nodes": nodes_leg, "edge": edge_leg, "esoftmax": esoftmax_leg, "heads": heads_leg, "gatheads": gatheads_leg, "gatv2": gatv2_leg, "fanout": fanout_leg, "blocks": blocks_leg, "bitnodes": bitnodes_leg, "affine": affine_leg, "codes": codes_leg}[args.leg]
        rows = leg(torch, QGTC, args.graphs.split(","), args.reps)
        if args.json:
            os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
            with open(args.json, "w") as f:
                json.dump(rows, f, indent=1)
        print(json.dumps({"tiled_bench_" + args.leg: [{k: v for k, v in r.items() if k != "agg"} for r in rows]}))
        return
    rows = []
    for name in args.graphs.split(","):
        n, deg = GRAPHS[name]
        t0 = time.time()
        g = make_sbm_graph(name, n, max(1, n // 128), deg, 1, seed=3)
        gen_s = time.time() - t0
        perm = np.random.default_rng(7).permutation(n)
        for order in ("block-local", "permuted", "reordered"):
            src, dst = (g.src, g.dst) if order == "block-local" else (perm[g.src], perm[g.dst])
            dsrc, ddst = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
            reorder = order == "reordered"
            pack_ms = timed(torch, lambda: QGTC.pack_edges_tiled(dsrc, ddst, n, False, reorder), max(3, args.reps // 3), warmup=1)
            adj = QGTC.pack_edges_tiled(dsrc, ddst, n, reorder=reorder)
            T = adj.n_tiles
            rec = {"graph": name, "order": order, "n": n, "edges": int(src.size), "gen_s": round(gen_s, 1), "pack_ms": round(pack_ms, 3),
                   "tiles": T, "tile_bytes": 512 * T, "max_block_tiles": adj.max_block_tiles, "agg": []}
            if reorder:
                rec["reorder_ms"] = round(timed(torch, lambda: QGTC.reorder_nodes(dsrc, ddst, n, validate=False), max(3, args.reps // 3),
                                                warmup=1), 3)
                print(f"{name:9s} {order:11s} reorder_nodes {rec['reorder_ms']:.3f} ms", flush=True)
            rng = np.random.default_rng(1)
            for N in (16, 64, 256):
                for w in (1, 2, 4):
                    X = QGTC.val2bit(torch.from_numpy(rng.integers(0, 2 ** w, size=(n, N)).astype(np.float32)).cuda(), w, True, False)
                    out = QGTC.tiledMM2Bit(adj, X, N, w, w)
                    ms = timed(torch, lambda: QGTC.tiledMM2Bit(adj, X, N, w, w), args.reps)
                    algo = 524 * T + X.numel() * 4 + out.numel() * 4
                    rec["agg"].append({"N": N, "w": w, "ms": round(ms, 4), "hbm_frac": round(algo / (ms * 1e-3) / HBM_BPS, 4)})
                    print(f"{name:9s} {order:11s} T={T:>10d} N={N:<4d} w={w} agg {ms:9.4f} ms  hbm {rec['agg'][-1]['hbm_frac']:.3f}",
                          flush=True)
                    del X, out
            if name == "arxiv" and not reorder:
                # the dense route of the same edge list: pack_edges + bitMM2Bit (n^2 / 8 bytes of adjacency)
                A = QGTC.pack_edges(dsrc, ddst, n, n, 1, False)
                dense = {"pack_ms": round(timed(torch, lambda: QGTC.pack_edges(dsrc, ddst, n, n, 1, False), 3, warmup=1), 3),
                         "adj_bytes": A.numel() * 4, "agg": []}
                for N, w in ((16, 1), (64, 2), (256, 4)):
                    X = QGTC.val2bit(torch.from_numpy(rng.integers(0, 2 ** w, size=(n, N)).astype(np.float32)).cuda(), w, True, False)
                    ms = timed(torch, lambda: QGTC.bitMM2Bit(A, X, n, n, N, 1, w, w), max(3, args.reps // 2))
                    assert torch.equal(QGTC.bitMM2Bit(A, X, n, n, N, 1, w, w), QGTC.tiledMM2Bit(adj, X, N, w, w))
                    dense["agg"].append({"N": N, "w": w, "ms": round(ms, 4)})
                    print(f"{name:9s} {order:11s} dense route N={N:<4d} w={w} agg {ms:9.4f} ms (pack {dense['pack_ms']} ms)", flush=True)
                    del X
                rec["dense"] = dense
                del A
            print(f"{name:9s} {order:11s} pack {pack_ms:.3f} ms  T={T}  tiles {512 * T / 2**20:.1f} MiB  edges {src.size}", flush=True)
            rows.append(rec)
            del adj, dsrc, ddst
            torch.cuda.empty_cache()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)
    print(json.dumps({"tiled_bench": [{k: v for k, v in r.items() if k != "agg"} for r in rows]}))


if __name__ == "__main__":
    main()
