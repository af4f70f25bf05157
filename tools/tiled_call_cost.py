"""Host cost of one tiled call, Python to launch: microseconds of issue time per call in a host-bound loop (4000 back-to-back calls,
best of 5; the per_call loop of tools/call_cost.py) on a 40-node adjacency and X [40, 16], where the kernels are negligible. One row
per mode of tiledMMFloat - scores per head and fixed-fanout samples (taken once, outside the loop) included -, one for each of the
four launchers of the bit products (tiledMM2Int / tiledMM2Bit, plain and with a row_scale), and one forward plus backward of
tiledAggregate (``.sum().backward()``, X and both scores requiring a gradient) for the plain sum and the three attention routes, each on
adj and adj.T.
    python tools/tiled_call_cost.py OUT.json"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import QGTC as Q
from qgtc_ppopp22_amd.fanout import sample_fanout
from qgtc_ppopp22_amd.tiled import node_bitmap

n, N, bit2 = 40, 16, 2
ring = torch.arange(n)
adj = Q.pack_edges_tiled(torch.cat([ring, torch.tensor([0, 5, 12])]).cuda(), torch.cat([(ring + 1) % n, torch.tensor([20, 33, 3])]).cuda(), n)
X = torch.randn(n, N, device="cuda")
bit_X = Q.val2bit(X.abs(), bit2, True, False)
scale, zeros = torch.rand(n, device="cuda"), torch.zeros(n, device="cuda")
mask = node_bitmap(torch.arange(n, device="cuda") % 3 != 0, n)
heads = (torch.zeros(n, 2, device="cuda"), torch.rand(n, 2, device="cuda"))
sample = sample_fanout(adj, 3, 7)
masked_sample = sample_fanout(adj, 3, 7, row_mask=mask, nbr_mask=mask)
Xg = X.clone().requires_grad_(True)
p1, q1, p2, q2 = (t.clone().requires_grad_(True) for t in (zeros, scale, *heads))
CALLS = {"plain": lambda a: Q.tiledMMFloat(a, X),
         "src_scale": lambda a: Q.tiledMMFloat(a, X, scale, scale),
         "edge_drop": lambda a: Q.tiledMMFloat(a, X, edge_drop=(0.25, 7)),
         "node_masks": lambda a: Q.tiledMMFloat(a, X, row_mask=mask, nbr_mask=mask),
         "max": lambda a: Q.tiledMMFloat(a, X, reduce="max"),
         "attn": lambda a: Q.tiledMMFloat(a, X, attn=(zeros, scale)),
         "attn 2 heads": lambda a: Q.tiledMMFloat(a, X, attn=heads),
         "fanout sum": lambda a: Q.tiledMMFloat(a, X, fanout=sample),
         "fanout max": lambda a: Q.tiledMMFloat(a, X, reduce="max", fanout=sample),
         "fanout attn": lambda a: Q.tiledMMFloat(a, X, attn=(zeros, scale), fanout=sample),
         "masked fanout sum": lambda a: Q.tiledMMFloat(a, X, fanout=masked_sample),
         "backward plain": lambda a: Q.tiledAggregate(a, Xg).sum().backward(),
         "backward attn": lambda a: Q.tiledAggregate(a, Xg, attn=(p1, q1)).sum().backward(),
         "backward attn 2 heads": lambda a: Q.tiledAggregate(a, Xg, attn=(p2, q2)).sum().backward(),
         "backward fanout attn": lambda a: Q.tiledAggregate(a, Xg, attn=(p1, q1), fanout=sample).sum().backward(),
         "tiledMM2Int": lambda a: Q.tiledMM2Int(a, bit_X, N, bit2),
         "tiledMM2Bit": lambda a: Q.tiledMM2Bit(a, bit_X, N, bit2, 2),
         "tiledMM2Int scaled": lambda a: Q.tiledMM2Int(a, bit_X, N, bit2, scale),
         "tiledMM2Bit scaled": lambda a: Q.tiledMM2Bit(a, bit_X, N, bit2, 2, scale)}


def per_call(fn, a, reps=4000):
    for _ in range(200):
        fn(a)
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn(a)
        best = min(best, (time.perf_counter() - t0) / reps * 1e6)   # host-side issue time
        torch.cuda.synchronize()
    return round(best, 3)


rows = [{"call": name, "view": view, "us_per_call": per_call(fn, a)} for name, fn in CALLS.items() for view, a in (("adj", adj), ("adj.T", adj.T))]
for r in rows:
    print(r, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
json.dump(rows, open(sys.argv[1], "w"), indent=1)
