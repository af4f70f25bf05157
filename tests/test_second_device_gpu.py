"""Tensors on cuda:1 while the current device stays 0: the device guard of the checked path (the lean path hands such a call over), the
per-device once-only setup and kernel-handle table (launch_common.hip.h), and the per-device stream pool of the multi-stream entries.
Skipped, with the reason, on a machine with one GPU."""
import numpy as np
import pytest

import stream_cases as sc
from qgtc_ppopp22_amd.shapes import cols_shape, rows_shape

pytestmark = pytest.mark.gpu

CASE_IDS = ["val2bit-rows", "checked_val2bit-rows", "val2bit-cols", "bitMM2Bit-fp4_one", "checked_bitMM2Bit-fp4_one", "bitMM2Bit-popcount",
            "bitMM2Int-fp4_one", "tiledMMFloat-adj-sym-N64", "tiledMMFloat-adjT-sym-N32", "tiledMM2Bit-adjT-N64"]


@pytest.fixture(scope="module")
def env1(qgtc, oracle):
    import torch

    if torch.cuda.device_count() < 2:
        pytest.skip(f"needs two GPUs, {torch.cuda.device_count()} visible")
    torch.cuda.set_device(0)
    return sc.env_of(qgtc, oracle, torch, "cuda:1")


def test_the_cases_exist():
    ids = {c.id for c in sc.CASES}
    assert set(CASE_IDS) <= ids, sorted(set(CASE_IDS) - ids)


@pytest.mark.parametrize("case_id", CASE_IDS)
def test_operator_on_the_second_device(env1, case_id):
    torch = env1.torch
    case = next(c for c in sc.CASES if c.id == case_id)
    live = case.build(env1)
    with sc.switches(env1.Q, live):
        for k in (1, 2):
            live.load(k)
            outs = live.outputs(live.run())
            assert all(o.device == env1.dev for o in outs) and torch.cuda.current_device() == 0
            torch.cuda.synchronize(env1.dev)
            sc.check([o.cpu() for o in outs], live.expected[k], f"{case_id} on cuda:1, content {k}", old=live.expected[k - 1])


def test_multistream_entries_on_the_second_device(env1):
    torch, Q, O = env1.torch, env1.Q, env1.O
    M, K, N, a, w, ob = 129, 513, 100, 3, 2, 5
    X, Wt = sc._mm_operands(O, M, K, N, a, w, 4100)
    bX = torch.from_numpy(X.view(np.int32)).reshape(rows_shape(M, K, a)).to(env1.dev)
    bW = torch.from_numpy(Wt.view(np.int32)).reshape(cols_shape(K, N, w)).to(env1.dev)
    outs = [torch.full(rows_shape(M, N, ob), sc.NAN_WORD, dtype=torch.int32, device=env1.dev) for _ in range(3)]
    Q.bitMM2Bit_enqueue_streams(outs, bX, bW, M, K, N, a, w, ob, 7)
    with torch.cuda.device(env1.dev):
        got = torch.stack(outs).cpu()
    assert torch.cuda.current_device() == 0
    sc.check(list(got), [O.bitmm2bit(X, Wt, M, K, N, a, w, ob)] * 3, "enqueue_streams on cuda:1")
    for mode in (0, 2):
        bg = Q.BatchedGemm([bX], [bW], [(M, K, N)], a, w, ob, mode, True)
        bg.run_per_problem(3)
        with torch.cuda.device(env1.dev):
            got = bg.outs[0].cpu()
        assert bg.outs[0].device == env1.dev and torch.cuda.current_device() == 0
        sc.check([got], [O.bitmm2int(X, Wt, M, K, N, a, w, True) if mode == 2 else O.bitmm2bit(X, Wt, M, K, N, a, w, ob)], f"run_per_problem mode {mode}")
