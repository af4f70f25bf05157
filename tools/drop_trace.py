"""Plain and masked sum launches on the reordered arxiv graph, for a kernel trace: per (N, view) 40 rounds of the plain launch and the
masked launch at rates 0, 0.1 and 0.5, in that order (rate 0 keeps every edge: the hash is computed and nothing is dropped).

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/drop_trace.py
    python tools/drop_trace.py --summarise OUT/<host>/<pid>_kernel_trace.csv SUMMARY.json     # medians per kernel, chunk count and rate
"""
import os
import sys


def summarise(trace_csv, out_json):
    import collections
    import csv
    import json
    import re

    import numpy as np

    seq = collections.defaultdict(list)
    for r in csv.DictReader(open(trace_csv)):
        if "k_tiled_mm_f32" in r["Kernel_Name"]:
            short = re.sub(r"\(anonymous namespace\)::", "", r["Kernel_Name"]).split("(")[0].replace("void ", "").replace(" >", ">")
            seq[(short, int(r["Grid_Size_Y"]) // int(r["Workgroup_Size_Y"]))].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    out = []
    for (k, gy), v in seq.items():
        v = np.array(v)
        rec = {"kernel": k, "column_chunks": gy, "dispatches": len(v)}
        if "Drop" in k:   # a masked kernel's dispatches come in the order rate 0, 0.1, 0.5
            for i, rate in enumerate((0.0, 0.1, 0.5)):
                rec[f"median_us_rate_{rate}"] = round(float(np.median(v[i::3])) / 1000, 1)
        else:
            rec["median_us"] = round(float(np.median(v)) / 1000, 1)
        out.append(rec)
    json.dump(out, open(out_json, "w"), indent=1)


if len(sys.argv) == 4 and sys.argv[1] == "--summarise":
    summarise(sys.argv[2], sys.argv[3])
    sys.exit(0)

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

import QGTC  # noqa: E402
from qgtc_ppopp22_amd.graph import make_sbm_graph  # noqa: E402
from tiled_bench import GRAPHS  # noqa: E402

n, deg = GRAPHS["arxiv"]
g = make_sbm_graph("arxiv", n, max(1, n // 128), deg, 1, seed=3)
perm = np.random.default_rng(7).permutation(n)
adj = QGTC.pack_edges_tiled(torch.from_numpy(perm[g.src]).cuda(), torch.from_numpy(perm[g.dst]).cuda(), n, reorder=True)
xr = np.random.default_rng(1)
for N in (64, 256):
    X = torch.from_numpy(xr.standard_normal((n, N)).astype(np.float32)).cuda()
    for a in (adj, adj.T):
        for _ in range(40):
            QGTC.tiledMMFloat(a, X)
            for rate in (0.0, 0.1, 0.5):
                QGTC.tiledMMFloat(a, X, edge_drop=(rate, 12345))
torch.cuda.synchronize()
print("done")
