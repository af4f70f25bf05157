"""The stream contract (tests/stream_contract.py) is complete: every name the built extension and the Python layer export is classified,
nothing in the table is stale, and every entry of the two asynchronous classes has a case the GPU tests run (tests/stream_cases.py).
No GPU: the extension imports without a device."""
import stream_cases
from stream_contract import ALIASES, ASYNC, CONTRACT, FORKS, HOST, PURE, exported_names, names_of

# the entries of the FORKS class are driven by tests/test_multistream_gpu.py, not by the generic probe
MULTISTREAM_TESTS = {"QGTC.bitMM2Bit_enqueue_streams": "test_enqueue_streams", "QGTC.BatchedGemm.run_per_problem": "test_run_per_problem"}


def test_every_exported_name_is_classified_once():
    exported = exported_names()
    missing = sorted(exported - set(CONTRACT))
    stale = sorted(set(CONTRACT) - exported)
    assert not missing, f"not in tests/stream_contract.py (classify them by reading the code): {missing}"
    assert not stale, f"tests/stream_contract.py names what no longer exists: {stale}"
    assert all(c in (ASYNC, FORKS, HOST, PURE) and why for c, why in CONTRACT.values())
    assert len(exported) >= 100


def test_aliases_are_the_same_objects():
    import QGTC

    for alias, target in ALIASES.items():
        assert getattr(QGTC, alias.split(".")[-1]) is getattr(QGTC, target.split(".")[-1]), alias
        assert CONTRACT[alias][0] == CONTRACT[target][0]
    assert QGTC.checked_bitMM2Bit is not QGTC.bitMM2Bit and QGTC.checked_val2bit is not QGTC.val2bit       # two call paths, both covered


def test_the_expected_members_are_where_the_issue_put_them():
    """The members the design names for each class (a reader moving one must say why here)."""
    for n in ("val2bit", "bit2val", "bitMM2Bit", "bitMM2Bit_col", "bitMM2Int", "bitMM2Bit_enqueue", "gcn_layer", "val2bit_many", "i8gemm",
              "tiledMM2Bit", "tiledMM2Int", "tiledMMFloat", "tiledAggregate", "BatchedGemm.run", "FusedLayer.run", "ChainedPair.run",
              "EpochPlan.run", "tile_occupancy"):
        assert CONTRACT["QGTC." + n][0] == ASYNC, n
    assert names_of(FORKS) == ["QGTC.BatchedGemm.run_per_problem", "QGTC.bitMM2Bit_enqueue_streams"]
    for n in ("pack_edges", "pack_edges_tiled", "reorder_nodes", "tile_counters", "bitMM2Bit_base_cnt", "bitMM2Bit_zerojump_cnt",
              "bitMM2Bit_profile", "i8gemm_profile", "profile", "BatchedGemm.occupied_fraction", "last_batched_violation", "EpochPlan.load",
              "EpochPlan.run_checked", "TiledAdjacency.max_block_tiles"):
        assert CONTRACT["QGTC." + n][0] == HOST, n
    assert CONTRACT["ext._tiled_pack"][0] == HOST


def test_every_asynchronous_entry_has_its_gpu_cases():
    """ASYNC: at least one case with an ordering probe and one with a capture test; FORKS: a test of its own."""
    for name in names_of(ASYNC):
        cases = stream_cases.cases_of(name)
        assert any(c.probe for c in cases), f"{name}: no ordering probe in tests/stream_cases.py"
        assert any(c.capture for c in cases), f"{name}: no capture case in tests/stream_cases.py"
    import test_multistream_gpu

    for name in names_of(FORKS):
        assert not stream_cases.cases_of(name), f"{name} forks streams: it is never captured"
        assert callable(getattr(test_multistream_gpu, MULTISTREAM_TESTS[name])), name
    named = {e for c in stream_cases.CASES for e in c.entries}
    unknown = sorted(e for e in named if not e.startswith("C.") and (e not in CONTRACT or CONTRACT[e][0] != ASYNC))
    assert not unknown, f"cases name entries that are not ASYNC in the contract: {unknown}"
    for entry in stream_cases.RAW_ENTRIES:
        assert any(c.raw for c in stream_cases.cases_of("C." + entry)), f"{entry}: no raw-entry case"
    ids = [c.id for c in stream_cases.CASES]
    assert len(ids) == len(set(ids))
