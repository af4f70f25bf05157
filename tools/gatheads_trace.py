"""The attention path with heads at (H, d) = (4, 64) on the reordered arxiv graph, for a kernel trace: 20 rounds of forward plus all three
gradients, the one call for all heads and then the loop over the heads, on adj (the shape where the one call is level
with the loop).

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/gatheads_trace.py
    python tools/gatheads_trace.py --summarise OUT/<host>/<pid>_kernel_trace.csv SUMMARY.json     # per kernel: dispatches a round, median us
"""
import os
import sys

ROUNDS, H, D = 20, 4, 64


def summarise(trace_csv, out_json):
    import collections
    import csv
    import json
    import re

    import numpy as np

    seq = collections.defaultdict(list)
    for r in csv.DictReader(open(trace_csv)):
        if "k_tiled_att" in r["Kernel_Name"] or "k_rowdot" in r["Kernel_Name"] or "k_tiled_max" in r["Kernel_Name"]:
            short = re.sub(r"\(anonymous namespace\)::", "", r["Kernel_Name"]).split("(")[0].replace("void ", "").replace(" >", ">")
            seq[(short, int(r["Grid_Size_Y"]) // int(r["Workgroup_Size_Y"]))].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    out = [{"kernel": k, "grid_y": gy, "dispatches_a_round": round(len(v) / (ROUNDS + 1), 2), "median_us": round(float(np.median(v)) / 1000, 1),
            "us_a_round": round(float(np.median(v)) / 1000 * len(v) / (ROUNDS + 1), 1)} for (k, gy), v in seq.items()]
    json.dump(sorted(out, key=lambda r: r["kernel"]), open(out_json, "w"), indent=1)


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
adj.T
xr = np.random.default_rng(1)
X, dY = (torch.from_numpy(xr.standard_normal((n, H * D)).astype(np.float32)).cuda() for _ in range(2))
P, Q = (torch.from_numpy(xr.uniform(-1, 1, (n, H)).astype(np.float32)).cuda() for _ in range(2))
Xg, Pg, Qg = (x.clone().requires_grad_(True) for x in (X, P, Q))
for _ in range(ROUNDS + 1):   # the first round is the warm-up; the summary divides by all of them alike
    torch.autograd.grad(QGTC.tiledAggregate(adj, Xg, attn=(Pg, Qg)), (Xg, Pg, Qg), dY)
    outs = [QGTC.tiledAggregate(adj, Xg[:, h * D:(h + 1) * D].contiguous(), attn=(Pg[:, h].contiguous(), Qg[:, h].contiguous())) for h in range(H)]
    torch.autograd.grad(torch.cat(outs, dim=1), (Xg, Pg, Qg), dY)
torch.cuda.synchronize()
print("done")
