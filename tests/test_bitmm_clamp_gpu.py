"""Every case of bitmm_clamp_cases.CLAMP_CASES on the device: the kernel its route query names, on sums next to the requantiser's clamp
and on both sides of it, against the oracle word for word (padding included) and against the NumPy rule element for element.
tests/test_bitmm_clamp_ledger.py (no GPU) shows which cells the table covers and that oracle and rule agree on these inputs, so a
mismatch here is the kernel's epilogue."""
import numpy as np
import pytest

import bitmm_clamp_cases as B
from helpers import to_dev, to_np_u32, use_engine
from qgtc_ppopp22_amd.shapes import cols_shape, rows_shape

pytestmark = pytest.mark.gpu


def _explain(c, got, what):
    """The first element that differs from the rule, with its sum and how far that is from 2^ob."""
    ref, s = B.reference(c), B.sums(c)
    bad = np.argwhere(got != ref)
    if not len(bad):
        return f"{what}: {B.case_id(c)}: the values agree with the rule; the packed words differ from the oracle's (padding?)"
    m, n = (int(v) for v in bad[0])
    return (f"{what}: {B.case_id(c)}: {len(bad)} of {ref.size} elements differ; first at ({m}, {n}): got {int(got[m, n])}, want {int(ref[m, n])}, "
            f"sum {int(s[m, n])} = 2^{c.ob} {int(s[m, n]) - (1 << c.ob):+d}")


@pytest.mark.parametrize("c", B.CLAMP_CASES, ids=[B.case_id(c) for c in B.CLAMP_CASES])
def test_outputs_next_to_the_clamp(qgtc, oracle, c):
    import torch
    from qgtc_ppopp22_amd import cabi

    lib = cabi.load()
    query = lib.qgtc_bitmm_route if c.form == "single" else lib.qgtc_bitmm_batched_route
    assert query(c.M, c.K, c.N, c.a, c.w, c.ob, c.mode, B.route_flags(c)).decode() == c.route
    qx, qw = B.operands(c)
    X, Wt = oracle.pack(B.as_int32(qx), c.a, False), oracle.pack(B.as_int32(qw), c.w, True)
    dX, dW = to_dev(torch, X, rows_shape(c.M, c.K, c.a)), to_dev(torch, Wt, cols_shape(c.K, c.N, c.w))
    cols = c.mode == 1
    prev_skip = qgtc.get_zero_skip()
    qgtc.set_zero_skip(c.zero_skip)
    try:
        with use_engine(qgtc, c.engine):
            if c.form == "single":
                outs = [(qgtc.bitMM2Bit_col if cols else qgtc.bitMM2Bit)(dX, dW, c.M, c.K, c.N, c.a, c.w, c.ob)]
            else:   # two problems on the same operands: the second workgroup row of the grid must give the same words
                bg = qgtc.BatchedGemm([dX, dX], [dW], [(c.M, c.K, c.N)] * 2, c.a, c.w, c.ob, c.mode, True, c.form == "grouped_jump")
                bg.run()
                outs = list(bg.outs)
            torch.cuda.synchronize()
    finally:
        qgtc.set_zero_skip(prev_skip)
    want_words = oracle.bitmm2bit(X, Wt, c.M, c.K, c.N, c.a, c.w, c.ob, col=cols)
    ref = B.reference(c)
    for i, out in enumerate(outs):
        assert tuple(out.shape) == (cols_shape(c.M, c.N, c.ob) if cols else rows_shape(c.M, c.N, c.ob))
        got = qgtc.bit2val(out, c.ob, c.M, c.N, cols, False).cpu().numpy().astype(np.int64)
        words = to_np_u32(out)
        assert np.array_equal(got, ref) and np.array_equal(words, want_words), _explain(c, got, f"problem {i}")
