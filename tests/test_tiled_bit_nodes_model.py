"""The inputs of the masked bit products' sweep (tests/tiled_bit_nodes_model.py), checked on the references alone: the sweep reaches
every launcher variant of both views and a second output chunk; the contract differs from every wrong rule of
tests/tiled_nodes_model.py in the float output and in the bit output; and the sums of the computed rows straddle requant's clamp, so
that a wrong sum cannot hide behind it. No GPU."""
import numpy as np
import pytest

import tiled_bit_nodes_model as bn
import tiled_nodes_model as nm
from tiled_model import FORWARD_VARIANTS, TRANSPOSED_VARIANTS, variant
from tiled_scaled_model import mean_scale

IDS = [f"n{n}-N{N}-{k}" for n, N, k in bn.SWEEP]


def test_the_sweep_reaches_every_launcher_variant_and_a_second_chunk():
    for transposed, variants in ((False, FORWARD_VARIANTS), (True, TRANSPOSED_VARIANTS)):
        assert sorted({variant(N, transposed) for N in bn.SWEEP_N}) == sorted(variants)
    assert max(bn.SWEEP_N) > 128 and max(bn.SWEEP_N) % 128 != 0
    assert len(bn.SWEEP) == 12 and {s[0] for s in bn.SWEEP} == set(bn.SWEEP_n) and {s[1] for s in bn.SWEEP} == set(bn.SWEEP_N)
    for kind in bn.KINDS:                          # every pair meets every n
        assert {s[0] for s in bn.SWEEP if s[2] == kind} == set(bn.SWEEP_n)
    for N in bn.SWEEP_N:                           # every output width, so every variant, runs under three of the four pairs
        assert len({s[2] for s in bn.SWEEP if s[1] == N}) == 3
    assert all(key in {(n, N) for n, N, _ in bn.SWEEP} for key in bn.EXTRA_BITS)
    assert sorted(bn.EXTRA_BITS.values()) == [(1, 1), (3, 3), (8, 8)]


@pytest.mark.parametrize("n,N,kind", bn.SWEEP, ids=IDS)
def test_the_contract_differs_from_every_wrong_rule(oracle, n, N, kind):
    """In the float output and in the bit output, on both views: under the case's own pair for the rules that pair can tell apart
    (tiled_bit_nodes_model.TELLS), and under two independent masks on the same graph and features for all four."""
    bit2, ob = bn.BITS
    src, dst, R, S, Xq = bn.inputs(n, N, kind, bit2)
    Rb, Sb = bn.pair(np.random.default_rng(n + N), n, "both")
    for transposed in (False, True):
        for rows, nbrs, rules in ((R, S, bn.TELLS[kind]), (Rb, Sb, nm.WRONG_RULES)):
            floats, bits = bn.reference(oracle, bn.sums(src, dst, n, Xq, rows, nbrs, transposed), ob)
            for wrong in rules:
                wf, wb = bn.reference(oracle, bn.sums(src, dst, n, Xq, rows, nbrs, transposed, wrong), ob)
                assert (floats != wf).any(), (wrong, transposed, "float output")
                assert (bits != wb).any(), (wrong, transposed, "bit output")


@pytest.mark.parametrize("n,N,kind", bn.SWEEP, ids=IDS)
def test_the_reference_sums_straddle_the_clamp(n, N, kind):
    """Of the sums of the computed rows at (bit2, output_bit) = (2, 3), on both views, at least 5 % lie strictly between 0 and 7 and at
    least 5 % at or above 7: otherwise requant hides a wrong sum. The pairs of EXTRA_BITS saturate far more; their fractions are
    printed, the condition does not rest on them."""
    for bit2, ob in bn.bit_pairs(n, N):
        src, dst, R, S, Xq = bn.inputs(n, N, kind, bit2)
        for transposed in (False, True):
            inside, top = bn.clamp_fractions(bn.sums(src, dst, n, Xq, R, S, transposed), R, ob)
            print(f"n={n} N={N} {kind} bits=({bit2}, {ob}) transposed={transposed}: in range {inside:.3f}, saturated {top:.3f}")
            if (bit2, ob) == bn.BITS:
                assert inside >= 0.05 and top >= 0.05, (transposed, inside, top)


def test_a_masked_out_row_is_a_row_without_neighbours(oracle):
    """What the contract says of a row outside row_mask, in the references: sum 0, so requant(0) = 0 in every plane, and under a scale
    the value quantiser of 0.0f * row_scale - 0 for every finite scale, the induced mean scale (0 for such a row) included."""
    n, N, kind = bn.SWEEP[0]
    bit2, ob = bn.BITS
    src, dst, R, S, Xq = bn.inputs(n, N, "both", bit2)
    for transposed in (False, True):
        C = bn.sums(src, dst, n, Xq, R, S, transposed)
        assert not C[~R].any() and C[R].any()
        deg = bn.sums(src, dst, n, np.ones((n, 1), np.int64), R, S, transposed)[:, 0]
        for scale in (None, mean_scale(deg), np.random.default_rng(1).uniform(0.25, 2.0, n).astype(np.float32)):
            floats, bits = bn.reference(oracle, C, ob, scale)
            assert (floats[~R].view(np.uint32) == 0).all()
            planes = bits.reshape(ob, -1, 4)[:, :n, :]
            assert not planes[:, ~R, :].any()
