"""The C entries with an EXPLICIT stream handle (ctypes, raw device pointers), while torch's current stream stays the default one: the
entry gets a side stream's handle and everything it launches - the hipMemsetAsync ahead of an atomic-OR kernel, scans, fills - must go
there. The probe of tests/stream_cases.py::ordering_probe with the outputs prefilled with NaN on the side stream and canaries behind them,
and the capture test with the capturing stream's handle. Bit for bit against the oracle and the models."""
import pytest

import stream_cases as sc

pytestmark = pytest.mark.gpu


def _params():
    out = [pytest.param(c, id=c.id) for c in sc.CASES if c.raw]
    out += [pytest.param(e, id=f"NO-CASE-{e}") for e in sc.RAW_ENTRIES if not any(c.raw for c in sc.cases_of("C." + e))]
    return out


@pytest.fixture(scope="module")
def env(qgtc, oracle):
    import torch

    return sc.env_of(qgtc, oracle, torch)


@pytest.mark.parametrize("case", _params())
def test_raw_entry_on_a_side_stream_it_is_handed(env, case):
    assert not isinstance(case, str), f"{case} has no raw-entry case"
    sc.ordering_probe(env.torch, env.Q, case.build(env), f"{case.entries[0]} [{case.id}]")


@pytest.mark.parametrize("case", _params())
def test_raw_entry_capture_and_replay(env, case):
    assert not isinstance(case, str), f"{case} has no raw-entry case"
    sc.capture_and_replay(env.torch, env.Q, case.build(env), f"{case.entries[0]} [{case.id}]")
