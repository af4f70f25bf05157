"""The ledger of uninitialised allocations ("Dirty memory").

Every ``torch::empty`` / ``empty_like`` of the binding (``csrc/qgtc_torch.cpp``) and every ``torch.empty`` / ``empty_like`` / ``new_empty`` of
``tiled.py``, ``fanout.py``, ``sampler.py``, ``driver.py`` and ``dist.py`` hands out memory whose words are UNDEFINED: the caching allocator returns
whatever the block held last. :data:`LEDGER` names, for each such site, what defines every element before anything reads it:

``written whole by X``            entry (or host code) X stores every element, pad rows and pad words included, on every path
``cleared by X, then accumulated`` X clears the buffer on its own stream before its kernels add into it
``host-filled``                   a host buffer the binding fills itself before it is copied or read

:func:`find_sites` finds the sites by regular expression; ``tests/test_allocation_ledger.py`` fails when a site is missing from the
ledger or a row of the ledger no longer matches a site, so a new allocation has to say who defines it.
"""
from __future__ import annotations

import pathlib
import re
from collections import Counter

ROOT = pathlib.Path(__file__).resolve().parents[1]
PKG = ROOT / "qgtc_ppopp22_amd"
FILES = {"qgtc_torch.cpp": PKG / "csrc" / "qgtc_torch.cpp", "tiled.py": PKG / "tiled.py", "fanout.py": PKG / "fanout.py", "sampler.py": PKG / "sampler.py",
         "driver.py": PKG / "driver.py", "dist.py": PKG / "dist.py"}

VERDICTS = ("written whole by ", "cleared by ", "host-filled")

_CPP_SITE = re.compile(r"torch::empty(?:_like)?\s*\(")
_PY_SITE = re.compile(r"(?:torch\.empty(?:_like)?|\.new_empty)\s*\(")
_ASSIGN = re.compile(r"([A-Za-z_]\w*)\s*=(?!=)")
# a definition at column 0: a return type, the name, the opening parenthesis; not a control statement, not a macro call
_CPP_FUNC = re.compile(r"^(?!(?:if|for|while|switch|return|else|using|typedef|struct|class|namespace|template)\b)[A-Za-z_][\w:<>,\s\*&]*?\b([A-Za-z_]\w*)\s*\($")
# a struct holds its members' sites under its own name; the module definition is a macro call
_CPP_STRUCT = re.compile(r"^(?:struct\s+([A-Za-z_]\w*)\s*\{|(?=PYBIND11_MODULE\()(PYBIND11_MODULE))")
_PY_FUNC = re.compile(r"^\s*def\s+([A-Za-z_]\w*)\s*\(")


def _strip_cpp(line: str) -> str:
    """The line without its // comment and without the contents of its string literals."""
    line = re.sub(r'"(?:\\.|[^"\\])*"', '""', line)
    return line.split("//", 1)[0]


def _strip_py(line: str) -> str:
    line = re.sub(r'"(?:\\.|[^"\\])*"|\'(?:\\.|[^\'\\])*\'', '""', line)
    return line.split("#", 1)[0]


def _cpp_function(lines: list[str], i: int) -> str:
    """The function whose body holds line i: the nearest line above, at column 0, that opens a definition."""
    for j in range(i, -1, -1):
        line = lines[j]
        if not line or line[0] in " \t}#/":
            continue
        m = _CPP_STRUCT.match(line) or _CPP_FUNC.match(line.split("(", 1)[0] + "(")
        if m:
            return next(g for g in m.groups() if g)
    return "<file>"


def _py_function(lines: list[str], i: int) -> str:
    """The innermost ``def`` above line i with a smaller indent."""
    indent = len(lines[i]) - len(lines[i].lstrip())
    for j in range(i - 1, -1, -1):
        m = _PY_FUNC.match(lines[j])
        if m and len(lines[j]) - len(lines[j].lstrip()) < indent:
            return m.group(1)
    return "<module>"


def _tensor(statement: str, at: int) -> str:
    """The variable a site is assigned to: the last ``name =`` before it in its statement (a ternary's two sites share theirs)."""
    names = _ASSIGN.findall(statement[:at])
    return names[-1] if names else "<expression>"


def find_sites(name: str) -> Counter:
    """Counter of (file, function, tensor) over the allocation sites of FILES[name]."""
    path = FILES[name]
    cpp = path.suffix == ".cpp"
    raw = path.read_text().split("\n")
    lines = [(_strip_cpp if cpp else _strip_py)(ln) for ln in raw]
    # inside docstrings a Python line may mention torch.empty: the files audited here do not, and the test would show a site without a row
    sites: Counter = Counter()
    for i, line in enumerate(lines):
        for m in (_CPP_SITE if cpp else _PY_SITE).finditer(line):
            # the statement so far: back to the previous line that ended one (a ';', a '{' or a '}' in C++; the line itself in Python)
            start = i
            if cpp:
                while start > 0 and not lines[start - 1].rstrip().endswith((";", "{", "}")) and lines[start - 1].strip():
                    start -= 1
            before = " ".join(lines[start:i]) + " " + line[: m.start()]
            fn = _cpp_function(raw, i) if cpp else _py_function(raw, i)
            sites[(name, fn, _tensor(before, len(before)))] += 1
    return sites


def all_sites() -> Counter:
    out: Counter = Counter()
    for name in FILES:
        out.update(find_sites(name))
    return out


W, C, H = "written whole by ", "cleared by ", "host-filled"
CPP, TILED, FANOUT, DIST = "qgtc_torch.cpp", "tiled.py", "fanout.py", "dist.py"

# (file, function or struct, tensor) -> one verdict per site of that name, in source order. What follows the verdict's opening words names
# the entry (include/qgtc.h) or the host code that defines every element before anything reads it, and the path that was read for it.
LEDGER = {
    # ---- the reference's operators ------------------------------------------------------------------------------------------------
    (CPP, "val2bit", "out"): [W + "qgtc_val2bit (cols layout: one kernel, a word per lane, pad lines included)",
                              C + "qgtc_val2bit (rows layout: the fill, then atomic ORs), then accumulated"],
    (CPP, "bit2val", "out"): [W + "qgtc_bit2val: one thread per element of [height, width]"],
    (CPP, "mm2bit_impl", "out"): [W + "qgtc_bitmm2bit with QGTC_OUT_COLS: every granule of the cols layout, pad lines as zeros",
                                  W + "qgtc_bitmm2bit: every 16-byte granule of the rows layout, pad rows and pad words as zeros"],
    (CPP, "profile_impl", "out"): [W + "qgtc_bitmm2bit_profile: the same launch as qgtc_bitmm2bit, reps times"],
    (CPP, "bitMM2Int", "out"): [W + "qgtc_bitmm2int: every element of [M, N]"],
    (CPP, "tile_counters", "buf"): [C + "qgtc_tile_counters (both counters), then accumulated by atomic adds; read by buf.cpu()"],
    (CPP, "pack_edges", "out"): [C + "qgtc_pack_edge_list (one fill of out, also without an edge), then accumulated",
                                 C + "qgtc_pack_edges (the fill of every plane), then accumulated"],
    (CPP, "pack_edges", "scratch"): [C + "qgtc_pack_edge_list (both scratch bitmaps), then accumulated; never leaves the call"],
    (CPP, "pack_edges", "bad"): [C + "qgtc_pack_edge_list before any kernel, then accumulated (atomic max); read by bad.item()"],
    (CPP, "i8gemm", "out"): [W + "qgtc_i8gemm: every element of [M, N]"],
    (CPP, "i8gemm_profile", "out"): [W + "qgtc_i8gemm_profile: qgtc_i8gemm, reps + 1 times"],
    (CPP, "val2bit_many", "out"): [W + "qgtc_val2bit_batched, cols layout jobs", C + "qgtc_val2bit_batched (rows layout jobs), then accumulated"],
    (CPP, "PYBIND11_MODULE", "occ"): [W + "qgtc_tile_occupancy: one wave per word, lane 0 stores the ballot"],
    (CPP, "host_parts", "o"): ["never read: a timing of the allocator alone, dropped at once"],
    (CPP, "host_parts", "out"): [W + "qgtc_bitmm2bit, before the timed bursts write it again"],
    # ---- the tiled adjacency ----------------------------------------------------------------------------------------------------
    (CPP, "tiled_pack", "row_ptr"): [C + "qgtc_tiled_count BEFORE its return without an edge, then written by k_tiled_row_ptr; row_ptr[nrb].item() sizes "
                                     "kquad and tiles, so a stale word here would be a wild size"],
    (CPP, "tiled_pack", "work"): [W + "qgtc_tiled_count (keys, sorted keys, flags; the rocPRIM temporary is the primitives' own) before "
                                  "qgtc_tiled_fill reads it; absent without an edge"],
    (CPP, "tiled_pack", "bad"): [C + "qgtc_tiled_count before its return without an edge, then accumulated; read by bad.item()"],
    (CPP, "tiled_pack", "kquad"): [W + "qgtc_tiled_fill: the first cell of every tile stores its k-quad; [0] without a tile"],
    (CPP, "tiled_pack", "tiles"): [C + "qgtc_tiled_fill (T * 512 bytes), then accumulated by atomic ORs; [0, 32, 4] without a tile"],
    (CPP, "reorder_nodes", "perm"): [W + "qgtc_reorder_nodes: k_reorder_perm, or k_reorder_identity without an edge or a sweep"],
    (CPP, "reorder_nodes", "rank"): [W + "qgtc_reorder_nodes: perm is a permutation, so rank[perm[i]] = i reaches every element"],
    (CPP, "reorder_nodes", "work"): [C + "qgtc_reorder_nodes (size, changed: the fills; the hub tables hkey / hcount: k_reorder_sweep clears a node's slots before it counts), "
                                     "then accumulated; keys, offsets, lists, labels and proposals are written by its kernels before they read them; absent without an edge"],
    (CPP, "reorder_nodes", "bad"): [C + "qgtc_reorder_nodes before every path, then accumulated; read by bad.item()"],
    (CPP, "tiled_mm_on", "out"): [W + "qgtc_tiledmm2int / _t / _scaled: every workgroup stores its rows below n, also of a block without a tile",
                                  W + "qgtc_tiledmm2bit / _t / _scaled: whole 16-byte granules from the LDS staging, rows past n and columns past N as zeros"],
    (CPP, "tiled_degrees", "out_deg"): [W + "qgtc_tiled_degrees: k_tiled_out_degree stores every row below n, 0 without a tile"],
    (CPP, "tiled_degrees", "in_deg"): [C + "qgtc_tiled_degrees, then accumulated by atomic adds (not launched without a tile)"],
    (CPP, "tiled_degrees", "out_inv"): [W + "qgtc_tiled_degrees: k_tiled_inv_degree, 0 where the degree is 0"],
    (CPP, "tiled_degrees", "in_inv"): [W + "qgtc_tiled_degrees: k_tiled_inv_degree behind the in-degree kernel on the same stream"],
    (CPP, "tiled_colindex", "col_ptr"): [C + "qgtc_tiled_colindex BEFORE its return without a tile, then written by k_tiled_col_index (every k-quad "
                                         "boundary, the runs of empty k-quads included): an index, read by every product of adj.T"],
    (CPP, "tiled_colindex", "col_tile"): [W + "qgtc_tiled_colindex: k_tiled_col_index, one element per sorted tile; [0] without a tile"],
    (CPP, "tiled_colindex", "col_rb"): [W + "qgtc_tiled_colindex: k_tiled_col_index, one element per sorted tile; [0] without a tile"],
    (CPP, "tiled_colindex", "work"): [W + "qgtc_tiled_colindex (keys, then rocPRIM's sorted keys) before k_tiled_col_index reads it; absent without a tile"],
    (CPP, "tiled_sum_on", "out"): [W + "qgtc_tiledmm_f32_edge_heads / _t: every row of the view, +0 times row_scale for a row without a cell",
                                   W + "qgtc_tiledmm_f32 / _src / _drop / _nodes and their _t twins: every row, +0 for a row without a neighbour, outside "
                                       "row_mask or emptied by edge_drop"],
    (CPP, "tiled_red_on", "out"): [W + "qgtc_tiledmax_f32 / qgtc_tiledsel_f32 and twins: every row, +0 for a row without a (kept) neighbour"],
    (CPP, "tiled_red_on", "win"): [W + "qgtc_tiledmax_f32 and twins: every element, -1 for a row without a (kept) neighbour"],
    (CPP, "tiled_att_on", "out"): [W + "qgtc_rowdot_f32: one DOT per row", W + "qgtc_tiledatt_f32 and twins, forward: every row, +0 without a neighbour",
                                   W + "qgtc_tiledatt_f32 and twins, backward: every row", W + "qgtc_tiledatt_grad_f32 and twins: every row's fold, +0 without a cell"],
    (CPP, "tiled_att_on", "m"): [W + "qgtc_tiledatt_f32 and twins, forward: L(att_own + M) for every row, M = +0 without a neighbour"],
    (CPP, "tiled_att_on", "iv"): [W + "qgtc_tiledatt_f32 and twins, forward: 0 for a row without a (kept) neighbour"],
    (CPP, "tiled_inv_sqrt_degree", "out"): [W + "qgtc_tiled_inv_sqrt_degree: one thread per element"],
    # ---- grouped launches -------------------------------------------------------------------------------------------------------
    (CPP, "BatchedGemm", "out_pool"): [W + "qgtc_bitmm_batched in run(): every problem's view whole; the up to three words between two views (each "
                                       "starts 16-byte aligned) belong to no view and are never read"],
    (CPP, "BatchedGemm", "occ_pool"): [W + "qgtc_tile_occupancy_batched in the constructor: lane 0 of every wave stores its ballot word"],
    (CPP, "BatchedGemm", "host"): [H + ": memcpy of the descriptors before host.to(dev)"],
    (CPP, "BatchedGemm", "stats"): [W + "k_occupancy_decide (both words) in the constructor; read by stats.cpu()"],
    (CPP, "EpochPlan", "occ_pool"): [W + "qgtc_tile_occupancy_batched in the constructor"],
    (CPP, "EpochPlan", "tile_pool"): [W + "qgtc_adj_tiles_from_rows per batch in the constructor"],
    (CPP, "EpochPlan", "xc"): [W + "qgtc_chain_from_cols in the constructor"],
    (CPP, "EpochPlan", "th"): [H + ": memcpy of the bitmap launch's descriptors before th.to(dev)"],
    (CPP, "EpochPlan", "stats"): [W + "k_occupancy_decide (both words) behind the bitmap launch; read by stats.cpu()"],
    (CPP, "EpochPlan", "host"): [H + ": memcpy of the batch table before host.to(dev)", H + ": memcpy of both tables of load() before host.to(dev)"],
    (CPP, "EpochPlan", "zero"): [C + "qgtc_load_batches (the bitmap route: all of it; the bucketed route: the statistics' 16 bytes, and every word of "
                                 "A is written once from LDS), then accumulated"],
    (CPP, "EpochPlan", "work"): [W + "qgtc_load_batches: k_load_sort fills offsets, buckets and counters before k_load_tiles reads them; four spare "
                                 "words on the bitmap route, never read"],
    (CPP, "EpochPlan", "tiles"): [W + "qgtc_load_batches when a_tiles; otherwise four spare words no descriptor names"],
    (CPP, "EpochPlan", "occ"): [W + "qgtc_load_batches: k_load_finish / k_load_tiles store every bitmap word"],
    (CPP, "EpochPlan", "xp"): [W + "qgtc_load_batches: k_load_x_cols / k_load_x_both, pad lines included"],
    (CPP, "EpochPlan", "xrp"): [W + "qgtc_load_batches with QGTC_LOAD_X_ROWS; otherwise four spare words no descriptor names"],
    (CPP, "EpochPlan", "xcp"): [W + "qgtc_load_batches with QGTC_LOAD_X_CHAIN; otherwise four spare words no descriptor names"],
    (CPP, "EpochPlan", "bad"): [C + "qgtc_load_batches before any kernel, then accumulated; read by bad.item()"],
    (CPP, "EpochPlan", "codes"): [W + "qgtc_expand_weights in bind()"],
    (CPP, "EpochPlan", "pool"): [W + "the plan's launches in run(): every stage output a later stage or outs() reads is written whole by the launch "
                                 "before it (qgtc_epoch_pool_layout sizes them)"],
    (CPP, "EpochPlan", "descs"): [W + "qgtc_epoch_plan_fill in bind(): one descriptor per (stage, batch)"],
    # ---- tiled.py -----------------------------------------------------------------------------------------------------------------
    (TILED, "_inv_degree", "out"): [W + "qgtc_tiled_inv_degree: one thread per element"],
    (TILED, "node_bitmap", "out"): [W + "qgtc_node_bitmap: every word, pad bits and pad words zero"],
    (TILED, "_value_index", "counts"): [W + "qgtc_tiled_value_index: one count per tile; [0] without a tile, where the entry is not called"],
    (TILED, "_value_index", "val_row"): [W + "qgtc_tiled_value_index: 32 prefixes per tile; [0, 32] without a tile"],
    (TILED, "edge_slots", "out"): [W + "qgtc_tiled_edge_slots: one slot or -1 per edge, -1 everywhere without a tile; [0] without an edge"],
    (TILED, "edge_endpoints", "row"): [W + "qgtc_tiled_edge_endpoints: one store per stored cell; [0] without a cell, where the entry is not called"],
    (TILED, "edge_endpoints", "col"): [W + "qgtc_tiled_edge_endpoints: one store per stored cell; [0] without a cell"],
    (TILED, "_sddmm", "out"): [W + "qgtc_tiled_sddmm_heads_f32: one store per (slot, head); [0, heads] without a cell, where the entry is not called"],
    (TILED, "sample_fanout", "thr"): [W + "qgtc_tiled_fanout_thr / _t / _nodes / _t_nodes: k_tiled_fanout_thr and k_tiled_fanout_thr_nodes run one wave per "
                                      "node below n (grid (n + 3) / 4 of four waves) and lane 0 stores thr[u] last, 0 where nothing is selected or walked"],
    (TILED, "sample_fanout", "counts"): [W + "qgtc_tiled_fanout_thr_nodes / _t_nodes: k_tiled_fanout_thr_nodes stores kept[u] beside thr[u] for every node "
                                         "below n, 0 outside row_mask (deg is 0 without a walk)"],
    (TILED, "_sum", "out"): [W + "qgtc_tiledmm_f32_fanout / _fanout_nodes and their _t twins: the entry bodies (qgtc_tiled_float*_fanout*.hip) call "
                             "tiled_mm_f32_masked, the launcher of qgtc_tiledmm_f32 (tiled_sum_on above), with the sample as the pack's mask: every row, "
                             "+0 for a row that keeps no neighbour"],
    (TILED, "_extremum", "out"): [W + "qgtc_tiledmax_f32_fanout / _fanout_nodes and their _t twins: the entry bodies (qgtc_tiled_max_fanout*.hip) call "
                                  "tiled_extremum_run, the launcher of qgtc_tiledmax_f32 (tiled_red_on above): every row, +0 without a kept neighbour"],
    (TILED, "_extremum", "arg"): [W + "qgtc_tiledmax_f32_fanout / _fanout_nodes and their _t twins, the same launch: every element, -1 without a kept "
                                  "neighbour; absent (NULL, 0 elements) without return_arg"],
    (TILED, "_att_heads_product", "out"): [W + "qgtc_tiledatt_heads_f32 and twins: every row and head, +0 without a (kept) neighbour; one head over a sample: "
                                           "qgtc_tiledatt_f32_fanout / _fanout_nodes and their _t twins, whose bodies (qgtc_tiled_attn*_fanout*.hip) call "
                                           "tiled_att_f32_run, the launcher of qgtc_tiledatt_f32 (tiled_att_on above)"],
    (TILED, "_att_heads_product", "m"): [W + "qgtc_tiledatt_heads_f32 and twins, forward: every (row, head); over a sample the same tiled_att_f32_run: "
                                         "L(att_own + M) for every row"],
    (TILED, "_att_heads_product", "inv"): [W + "qgtc_tiledatt_heads_f32 and twins, forward: 0 without a (kept) neighbour; over a sample the same "
                                           "tiled_att_f32_run"],
    (TILED, "_att_heads_grad", "out"): [W + "qgtc_tiledatt_grad_heads_f32 and twins: every (row, head), +0 without a cell; one head over a sample: "
                                        "qgtc_tiledatt_grad_f32_fanout / _fanout_nodes and their _t twins, whose bodies call tiled_att_grad_run, the "
                                        "launcher of qgtc_tiledatt_grad_f32 (tiled_att_on above)"],
    (TILED, "_att_heads_rowdot", "out"): [W + "qgtc_rowdot_heads_f32: one DOT per (row, head)"],
    (TILED, "_edge_softmax", "alpha"): [W + "qgtc_tiled_edge_softmax_heads_f32 / _t: one store per (slot, head); empty without a cell"],
    (TILED, "_edge_softmax", "m"): [W + "qgtc_tiled_edge_softmax_heads_f32 / _t: every (node, head); the entry's own clear (tiled_esm_no_cells) without a cell"],
    (TILED, "_edge_softmax", "inv"): [W + "qgtc_tiled_edge_softmax_heads_f32 / _t: every (node, head); the entry's own clear without a cell"],
    (TILED, "_edge_softmax_grad", "out"): [W + "qgtc_tiled_edge_softmax_grad_heads_f32 / _t: one store per (slot, head); empty without a cell, not called"],
    (TILED, "_addscore", "out"): [W + "qgtc_tiled_addscore_heads_f32: one store per (slot, head); [0, heads] without a cell, not called"],
    (TILED, "_addscore_grad", "d_own"): [W + "qgtc_tiled_addscore_grad_heads_f32 / _t: every owner's fold, +0 without a cell (torch.zeros_like when nnz is 0)"],
    (TILED, "_addscore_grad", "P"): [W + "qgtc_tiled_addscore_grad_heads_f32 / _t: every owner's fold, +0 without a cell"],
    # ---- fanout.py ---------------------------------------------------------------------------------------------------------------
    (FANOUT, "frontier", "out"): [W + "qgtc_tiled_fanout_frontier / _t: k_tiled_fanout_frontier (grid S128(n), threads 0 .. 3 store the k-quad's four "
                                  "words) and k_tiled_fanout_frontier_t (grid S128(n) * 4, thread 0 stores the block's word) store every word after the "
                                  "barrier, also without a tile; pad bits cleared by tiled_blocks_valid"],
    # ---- dist.py (multi-GPU: in the ledger only) ----------------------------------------------------------------------------------
    (DIST, "gather_batch_summaries", "out"): [W + "dist.all_gather_into_tensor: world equal shards"],
    (DIST, "gather_replica_summaries", "out"): [W + "dist.all_gather_into_tensor: world equal shards"],
    (DIST, "gather_batch_outputs", "all_n"): [W + "dist.all_gather_into_tensor before all_n.max().item()"],
    (DIST, "gather_batch_outputs", "allbuf"): [W + "dist.all_gather_into_tensor of zero-padded buffers"],
}

# sites nothing reads: the one verdict outside the three
NEVER_READ = {(CPP, "host_parts", "o")}

# torch::zeros / zeros_like sites of the binding, (function, tensor) -> the sentence of include/qgtc.h that makes the CALLER responsible for
# clearing that argument. The only zero-filled allocations the contract allows; none today.
ZERO_FILLED = {}


def check(sites=None):
    """(missing, stale, malformed): sites without a row (or with fewer verdicts than sites), rows without a site, verdicts outside
    VERDICTS. All empty when the ledger matches the sources."""
    sites = all_sites() if sites is None else sites
    missing = sorted(k for k, n in sites.items() if len(LEDGER.get(k, ())) != n)
    stale = sorted(k for k in LEDGER if k not in sites)
    malformed = sorted(k for k, rows in LEDGER.items() for v in rows
                       if not (v.startswith(VERDICTS[:2]) or v.startswith(VERDICTS[2]) or (k in NEVER_READ and v.startswith("never read")))
                       or (v.startswith(VERDICTS[1]) and "then accumulated" not in v and "then written" not in v))
    return missing, stale, malformed


if __name__ == "__main__":
    for key, count in sorted(all_sites().items()):
        print(key, count)
