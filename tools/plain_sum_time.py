"""Plain tiledMMFloat sum on the reordered arxiv / reddit SBM graphs, N = 64 and 256, both views: two passes, medians in ms.
    python tools/plain_sum_time.py OUT.json"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import QGTC  # noqa: E402
from qgtc_ppopp22_amd.graph import make_sbm_graph  # noqa: E402
from tiled_bench import GRAPHS, timed_alternating  # noqa: E402

rows = []
for name in ("arxiv", "reddit"):
    n, deg = GRAPHS[name]
    g = make_sbm_graph(name, n, max(1, n // 128), deg, 1, seed=3)
    perm = np.random.default_rng(7).permutation(n)
    dsrc, ddst = torch.from_numpy(perm[g.src]).cuda(), torch.from_numpy(perm[g.dst]).cuda()
    adj = QGTC.pack_edges_tiled(dsrc, ddst, n, reorder=True)
    t = adj.T
    xr = np.random.default_rng(1)
    for N in (64, 256):
        X = torch.from_numpy(xr.standard_normal((n, N)).astype(np.float32)).cuda()
        for a, direction in ((adj, "forward"), (t, "transposed")):
            for p in range(2):
                (ms,) = timed_alternating(torch, [lambda: QGTC.tiledMMFloat(a, X)], 30)
                rows.append({"graph": name, "N": N, "direction": direction, "pass": p, "plain_ms": ms})
                print(rows[-1], flush=True)
        del X
    del adj, t
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
json.dump(rows, open(sys.argv[1], "w"), indent=1)
