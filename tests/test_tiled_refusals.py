"""The refusals of QGTC.tiledMMFloat and QGTC.tiledAggregate, one fault per call: which combinations of ``reduce``, ``attn``, the scales,
``return_arg``, ``return_stats``, ``edge_drop``, the node masks and ``edge_weight`` are refused, with which exception type and which
message. Every call is stopped in the Python layer, on an adjacency of CPU tensors (no GPU needed). Both functions run the same table;
``return_arg`` and ``return_stats`` are tiledMMFloat's arguments only."""
import pytest
import torch

import qgtc_ppopp22_amd.tiled as tiled

N_NODES, N_FEATS = 40, 8
MASK_WORDS = (N_NODES + 127) // 128 * 4


@pytest.fixture(scope="module")
def cpu_adj():
    n = N_NODES
    return tiled.TiledAdjacency(n, torch.zeros((n + 31) // 32 + 1, dtype=torch.int64), torch.zeros(0, dtype=torch.int32),
                                torch.zeros((0, 32, 4), dtype=torch.int32))


def _scale():
    return torch.ones(N_NODES)


def _attn():
    return (torch.zeros(N_NODES), torch.zeros(N_NODES))


def _mask(dtype=torch.int32, words=MASK_WORDS):
    return torch.zeros(words, dtype=dtype)


def _weights():
    return torch.zeros(0)   # the adjacency stores no cell


NOT_BUILT = "cannot be combined with {}: not built"
# (id, keyword arguments, exception type, match, tiledMMFloat only)
FAULTS = [
    ("reduce-unknown", dict(reduce="mean"), ValueError, 'reduce must be "sum", "max" or "min", not \'mean\'', False),
    ("row_scale-with-max", dict(row_scale=_scale(), reduce="max"), ValueError, 'row_scale cannot be combined with reduce="max"', False),
    ("src_scale-with-min", dict(src_scale=_scale(), reduce="min"), ValueError, 'src_scale cannot be combined with reduce="min"', False),
    ("row_scale-with-attn", dict(row_scale=_scale(), attn=_attn()), ValueError, "row_scale cannot be combined with attn", False),
    ("src_scale-with-attn", dict(src_scale=_scale(), attn=_attn()), ValueError, "src_scale cannot be combined with attn", False),
    ("attn-with-max", dict(attn=_attn(), reduce="max"), ValueError, 'attn cannot be combined with reduce="max"', False),
    ("return_arg-with-sum", dict(return_arg=True), ValueError, 'return_arg needs reduce="max" or "min"', True),
    ("return_arg-with-attn", dict(return_arg=True, attn=_attn()), ValueError, "return_arg cannot be combined with attn", True),
    ("return_stats-without-attn", dict(return_stats=True), ValueError, "return_stats needs attn", True),
    ("slope-2", dict(attn=_attn(), negative_slope=2.0), ValueError, r"negative_slope must lie in \[0, 1\], not 2\.0", False),
    ("slope-nan", dict(attn=_attn(), negative_slope=float("nan")), ValueError, r"negative_slope must lie in \[0, 1\], not nan", False),
    ("edge_drop-not-a-pair", dict(edge_drop=(0.5,)), TypeError, r"edge_drop must be a pair \(rate, seed\) or None", False),
    ("edge_drop-rate-1", dict(edge_drop=(1.0, 3)), ValueError, r"edge_drop's rate must lie in \[0, 1\), not 1\.0", False),
    ("edge_drop-rate-nan", dict(edge_drop=(float("nan"), 3)), ValueError, r"edge_drop's rate must lie in \[0, 1\), not nan", False),
    ("edge_drop-rate-bool", dict(edge_drop=(True, 3)), TypeError, r"edge_drop's rate must be a float in \[0, 1\), not bool", False),
    ("edge_drop-seed-negative", dict(edge_drop=(0.5, -1)), ValueError, r"edge_drop's seed must lie in \[0, 2\^64\), not -1", False),
    ("edge_drop-seed-2^64", dict(edge_drop=(0.5, 1 << 64)), ValueError, r"edge_drop's seed must lie in \[0, 2\^64\), not 18446744073709551616",
     False),
    ("edge_drop-seed-float", dict(edge_drop=(0.5, 3.0)), TypeError, r"edge_drop's seed must be an int in \[0, 2\^64\), not float", False),
    ("row_mask-dtype", dict(row_mask=_mask(torch.int64)), TypeError, r"row_mask must be int32 \(tiled\.node_bitmap\), not torch\.int64", False),
    ("nbr_mask-dtype", dict(nbr_mask=_mask(torch.bool)), TypeError, r"nbr_mask must be int32 \(tiled\.node_bitmap\), not torch\.bool", False),
    ("row_mask-length", dict(row_mask=_mask(words=MASK_WORDS + 1)), ValueError,
     rf"row_mask must have shape \[{MASK_WORDS}\] \(S128\(n\) \* 4 words\), not \[{MASK_WORDS + 1}\]", False),
    ("nbr_mask-length", dict(nbr_mask=_mask(words=MASK_WORDS - 1)), ValueError,
     rf"nbr_mask must have shape \[{MASK_WORDS}\] \(S128\(n\) \* 4 words\), not \[{MASK_WORDS - 1}\]", False),
    ("row_mask-with-edge_drop", dict(row_mask=_mask(), edge_drop=(0.5, 3)), ValueError,
     "row_mask / nbr_mask " + NOT_BUILT.format("edge_drop"), False),
    ("nbr_mask-with-edge_drop", dict(nbr_mask=_mask(), edge_drop=(0.0, 0)), ValueError,
     "row_mask / nbr_mask " + NOT_BUILT.format("edge_drop"), False),
    ("edge_weight-with-src_scale", dict(edge_weight=_weights(), src_scale=_scale()), ValueError,
     "edge_weight " + NOT_BUILT.format("src_scale"), False),
    ("edge_weight-with-edge_drop", dict(edge_weight=_weights(), edge_drop=(0.5, 3)), ValueError,
     "edge_weight " + NOT_BUILT.format("edge_drop"), False),
    ("edge_weight-with-row_mask", dict(edge_weight=_weights(), row_mask=_mask()), ValueError,
     "edge_weight " + NOT_BUILT.format("row_mask / nbr_mask"), False),
    ("edge_weight-with-nbr_mask", dict(edge_weight=_weights(), nbr_mask=_mask()), ValueError,
     "edge_weight " + NOT_BUILT.format("row_mask / nbr_mask"), False),
    ("edge_weight-with-max", dict(edge_weight=_weights(), reduce="max"), ValueError, "edge_weight " + NOT_BUILT.format('reduce="max"'),
     False),
    ("edge_weight-with-attn", dict(edge_weight=_weights(), attn=_attn()), ValueError, "edge_weight " + NOT_BUILT.format("attn"), False),
]


CASES = [pytest.param(fn_name, *row[1:4], id=f"{fn_name}-{row[0]}") for fn_name in ("tiledMMFloat", "tiledAggregate") for row in FAULTS
         if fn_name == "tiledMMFloat" or not row[4]]   # return_arg and return_stats are arguments of tiledMMFloat only


@pytest.mark.parametrize("fn_name, kw, exc, match", CASES)
def test_a_single_fault_is_refused(cpu_adj, fn_name, kw, exc, match):
    X = torch.ones(N_NODES, N_FEATS)
    with pytest.raises(exc, match=match):
        getattr(tiled, fn_name)(cpu_adj, X, **kw)


def test_the_table_covers_what_it_says():
    """Every keyword that takes part in a refusal appears in the table, and the ids are distinct."""
    ids = [row[0] for row in FAULTS]
    assert len(set(ids)) == len(ids)
    named = set().union(*(row[1].keys() for row in FAULTS))
    assert named == {"reduce", "row_scale", "src_scale", "attn", "return_arg", "return_stats", "negative_slope", "edge_drop", "row_mask",
                     "nbr_mask", "edge_weight"}
