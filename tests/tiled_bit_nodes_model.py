"""The inputs and the exact references of node masks on the quantised tiled products (include/qgtc_bitnodes.h; ``row_mask=`` /
``nbr_mask=`` of QGTC.tiledMM2Bit / QGTC.tiledMM2Int): masking is restricting the edge list, so the reference is
tests/tiled_nodes_model.py's ``induced_edges`` followed by the existing exact models - ``tiled_model.aggregate`` / ``expected_bits`` /
``expected_floats``, and ``tiled_scaled_model.scaled`` / ``expected_bits_scaled`` under a ``row_scale``. Shared by the CPU test of the
inputs and the GPU tests, so that both see the same graphs, masks and features. No GPU."""
import numpy as np

import tiled_nodes_model as nm
from tiled_model import aggregate, expected_bits, expected_floats, random_edges
from tiled_scaled_model import expected_bits_scaled, scaled

KINDS = ("both", "rows", "nbrs", "same")           # (random, random), (random, none), (none, random), one mask twice
SWEEP_n = (97, 333, 1000)                          # n % 32 and n % 128 are nonzero
SWEEP_N = (8, 24, 40, 130)                         # R = 2, 4, 8, 16 on adj and 8, 16, 32, 64 on adj.T; 130 is a second 128-column chunk
SWEEP = [(n, N, KINDS[(iN + i) % 4]) for iN, N in enumerate(SWEEP_N) for i, n in enumerate(SWEEP_n)]
BITS = (2, 3)                                      # (bit2, output_bit) of every case: the pair the clamp condition rests on
EXTRA_BITS = {(97, 8): (1, 1), (333, 40): (3, 3), (1000, 130): (8, 8)}     # run beside BITS at one shape each: they saturate far more

# the wrong rules a kind of mask pair can tell from the contract: with one mask absent the rule that ignores the other set is the
# contract itself, and with one mask given twice so is the swap
TELLS = {"both": nm.WRONG_RULES, "rows": ("swapped", "nbrs_only", "lsb_first"), "nbrs": ("swapped", "rows_only", "lsb_first"),
         "same": ("rows_only", "nbrs_only", "lsb_first")}


def pair(rng, n, kind):
    """(R, S) bool [n] or None each, of density 0.5"""
    a, b = rng.random(n) < 0.5, rng.random(n) < 0.5
    return {"both": (a, b), "rows": (a, None), "nbrs": (None, b), "same": (a, a)}[kind]


def inputs(n, N, kind, bit2):
    """(src, dst, R, S, Xq) of a sweep case: the graph and the masks depend on (n, N, kind) alone, the features on bit2 too"""
    rng = np.random.default_rng(17 * n + N)
    src, dst = random_edges(rng, n, 6 * n + 5)
    R, S = pair(rng, n, kind)
    Xq = np.random.default_rng(1000 * n + 10 * N + bit2).integers(0, 2 ** bit2, size=(n, N))
    return src, dst, R, S, Xq


def bit_pairs(n, N):
    return (BITS,) + ((EXTRA_BITS[(n, N)],) if (n, N) in EXTRA_BITS else ())


def sums(src, dst, n, Xq, R, S, transposed, wrong=None):
    """the exact int64 sums [n, N] of the masked product on a view (``wrong``: under one of tiled_nodes_model.WRONG_RULES instead)"""
    return aggregate(*nm.induced_edges(src, dst, n, R, S, transposed, wrong), n, Xq, transposed)


def reference(oracle, C, ob, scale=None):
    """(float32 [n, N], rows-layout words) the masked tiledMM2Int / tiledMM2Bit must give for the sums C"""
    if scale is None:
        return expected_floats(C), expected_bits(oracle, C, ob)
    y = scaled(C, scale)
    return y, expected_bits_scaled(oracle, y, ob)


def clamp_fractions(C, R, ob):
    """(in range, saturated) fractions of the sums of the computed rows: strictly between 0 and 2^ob - 1 (for ob = 1: zero), and at or
    above 2^ob - 1"""
    c = np.asarray(C)[np.ones(len(C), bool) if R is None else R]
    top = 2 ** ob - 1
    inside = (c == 0) if ob == 1 else ((c > 0) & (c < top))
    return float(inside.mean()), float((c >= top).mean())
