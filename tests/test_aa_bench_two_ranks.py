"""`bench.py --gpus 2 --full` end to end on the one-GPU box: the parent starts two rank processes, both bind cuda:0 (test hook
QGTC_BENCH_SHARE_GPU) and talk over gloo (RCCL refuses two ranks on one device) - the whole N > 1 flow of main(): timed region with
barriers, max over ranks, checksum gather, the strong- and the weak-scaled epoch legs with their end-of-epoch gathers, ONE line from
rank 0. What the driver runs on an 8-GPU node as `--gpus 2 / 4 / 8` (BASELINE.json configs[4]) with backend nccl. And a plain
`bench.py --gpus 1`: the headline alone, and the output of its last timed step."""
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# The two ranks share the parent's stdout and gloo writes its announcement in pieces, so two announcements can arrive interleaved
# ("[Gloo] Rank [Gloo] Rank 0 is connected to 11 peer ranks.  is connected to ..."): then the text is still made of those pieces alone.
GLOO_PIECES = re.compile(r"(?:\[Gloo\] Rank |\d+| is connected to | peer ranks\. |Expected number of connected peer ranks is : |\s)*")


@pytest.mark.gpu
@pytest.mark.parametrize("gather", ["summaries", "outputs"])
def test_bench_with_two_ranks_sharing_the_gpu(gather, tmp_path):
    env = dict(os.environ, QGTC_BENCH_SHARE_GPU="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    extras = str(tmp_path / f"qgtc_bench2_{gather}.json")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--steps", "10", "--warmup", "3",
                          "--full", "--gather", gather, "--extras-file", extras], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    # gloo announces its ranks on stdout; nothing else but the line
    assert all(l.startswith("[Gloo]") for l in lines[:-1]) or GLOO_PIECES.fullmatch("\n".join(lines[:-1])), out.stdout[-2000:]
    assert len(lines[-1]) < 4096                                                # rank 0 only, one short line, LAST
    line = json.loads(lines[-1])
    assert line["n_gpus"] == 2 and line["ranks_seen"] == 2 and line["steps"] == 10 and line["scaling"] == "weak" and line["value"] > 0
    ex = json.load(open(extras))
    assert len(ex["rank_checksums"]) == 2 and all(c != 0 for c in ex["rank_checksums"])   # (int32 words summed: every output bit is set here)
    strong, weak = ex["cluster_gcn_epoch_ogbn_arxiv_shape"], ex["cluster_gcn_epoch_ogbn_arxiv_shape_weak_scaled"]
    assert strong["gathered_batches"] == 75 and weak["gathered_batches"] == 150             # 75 round-robin; 75 per rank
    assert strong["batched_correct_chain_ms"] > 0 and weak["batches_per_second"] > 0
    assert ex["batched_gin_epoch_ppi_shape_4bit"]["gathered_batches"] == 75
    if gather == "outputs":
        assert strong["gathered_output_bytes"] > 75 * 1100 * 10 * 4


@pytest.mark.gpu
def test_plain_bench_times_the_headline_and_dumps_its_last_step(oracle, tmp_path):
    """Without --full: one line with the contract's fields and nothing measured beside them, exactly --steps timed steps, and
    --dump-outputs writes the words of the last step - the C oracle's words for the seeded inputs."""
    import types

    import numpy as np

    from benchmarks.common import make_workload

    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    dump = tmp_path / "outputs"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                          "--dump-outputs", str(dump)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout[-2000:]
    line = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 7 and line["warmup"] == 2 and line["n_gpus"] == 1 and line["unit"] == "TOPS" and line["higher_is_better"] is True
    assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(7 * 2.0 * 4096 * 4096 * 64 / (line["ms_per_step"] * 7e-3) / 1e12, rel=1e-3)
    assert not {"roofline", "cpu_baseline", "parity_vs_oracle", "extras_file", "rccl_world1"} & set(line)
    assert sorted(os.listdir(dump)) == ["bitMM2Bit_out.npy"]
    got = np.load(dump / "bitMM2Bit_out.npy")
    assert got.dtype == np.float64 and got.nbytes <= 64 << 20
    M = K = 4096
    A, X, _, _ = make_workload(types.SimpleNamespace(val2bit=lambda *a: None), M, K, 64, 1, "cpu", seed=3)
    ref = oracle.bitmm2bit(oracle.val2bit(A.numpy(), 1), oracle.val2bit(X.numpy(), 1, True), M, K, 64, 1, 1, 1)
    np.testing.assert_array_equal(got.astype(np.int32).view(np.uint32).reshape(-1), ref)
