"""Profile target for the node reordering: QGTC.reorder_nodes on a shuffled SBM graph of tools/tiled_bench.py's sizes, with kernels
under their own names (k_reorder_*, rocPRIM's sort kernels), for one `rocprofv3 --kernel-trace --stats` run:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 tools/reorder_profile.py products 3

Prints one JSON line: the graph, the edges, and the wall time of each call (device-synchronised).
"""
from __future__ import annotations

import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main() -> None:
    name = sys.argv[1] if len(sys.argv) > 1 else "products"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    import torch

    import QGTC
    from qgtc_ppopp22_amd.graph import make_sbm_graph
    from tiled_bench import GRAPHS

    n, deg = GRAPHS[name]
    g = make_sbm_graph(name, n, max(1, n // 128), deg, 1, seed=3)
    p = np.random.default_rng(7).permutation(n)
    src, dst = torch.from_numpy(p[g.src]).cuda(), torch.from_numpy(p[g.dst]).cuda()
    ms = []
    for _ in range(reps + 1):   # the first call loads code objects
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        QGTC.reorder_nodes(src, dst, n, validate=False)
        torch.cuda.synchronize()
        ms.append(round((time.perf_counter() - t0) * 1e3, 2))
    print(json.dumps({"graph": name, "n": n, "edges": int(src.numel()), "warmup_ms": ms[0], "ms": ms[1:]}))


if __name__ == "__main__":
    main()
