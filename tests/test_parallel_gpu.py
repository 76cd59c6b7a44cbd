"""Multi-rank frame data parallelism on the REAL encoder: N ranks share the one GPU of the test box
(gloo carries the collective; on an 8-GPU node the same code runs over RCCL), every rank checks that the gathered
pooled tokens are bit-identical to the single-rank result — equal shards, ragged frame counts, an idle rank, and the
frames mode.  Also launches bench.py exactly as the driver does for N > 1 (tiny config) to keep that path alive."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, world, port, extra_env=None, timeout=600):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0", **(extra_env or {}))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(port)] + args
    return subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)


@pytest.mark.parametrize("world", [2, 3])
def test_encode_clips_dp_real_encoder_bit_identical(world):
    r = _run([os.path.join(ROOT, "tests", "dp_worker.py")], world, 29611 + world)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    for rank in range(world):
        assert f"DP_OK rank {rank}/{world}" in r.stdout, r.stdout[-2000:]


def test_bench_multi_rank_launch_path():
    """`python -m torch.distributed.run --nproc-per-node N bench.py --gpus N ...` as the driver launches it, two ranks
    on one device: both prefill modes produce one JSON line on rank 0 with n_gpus = 2 and the whole-job frame count."""
    for mode in ("sharded", "replicated"):
        r = _run([os.path.join(ROOT, "bench.py"), "--gpus", "2", "--config", "tiny", "--steps", "2", "--warmup", "1", "--prefill", mode,
                  "--no-cpu-baseline", "--traffic", "none"], 2, 29631,
                 extra_env={"VALLEY_BENCH_SAME_DEVICE": "1", "VALLEY_BENCH_BACKEND": "gloo"})
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(line) == 1, r.stdout[-2000:]
        j = json.loads(line[0])
        assert j["n_gpus"] == 2 and j["scaling"] == "weak" and j["value"] > 0
        assert j["config"]["parallelism"].startswith("frame-dp2") and ("replicated" in j["config"]["parallelism"]) == (mode == "replicated")
        # the N > 1 line carries what the north star's scaling target is read from (round 4): the aggregate encode rate over
        # all ranks and the all-gather's share of the step
        d = j["dist"]
        assert d["world_size"] == 2 and d["allgather_calls"] == 2
        assert d["vit_frames_per_s_all_gpus"] > 0 and abs(d["vit_frames_per_s_all_gpus"] - 2 * d["vit_frames_per_s_per_gpu_min"]) < 1.0
        assert 0 < d["allgather_share_of_step"] < 1


def test_bench_self_launch_defaults_to_configs3():
    """`python bench.py --gpus 2` with NO launcher: the script re-executes itself under torch.distributed.run, and at
    N > 1 its default workload is BASELINE configs[3] as written (c4: 32 frames x 8 clips per GPU, 13B prefill REPLICATED over all
    N x 8 sequences); with --full, the sharded-prefill (weak scaling) form of the same step is measured in the same run under
    also.sharded_prefill.  Two ranks share the one GPU of the test box (gloo carries the gather)."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", VALLEY_BENCH_SAME_DEVICE="1", VALLEY_BENCH_BACKEND="gloo")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--full"], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=2400)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(line) == 1, r.stdout[-2000:]
    j = json.loads(line[0])
    assert j["n_gpus"] == 2 and j["value"] > 0 and j["steps"] == 3
    assert j["config"]["name"] == "c4" and "32 frames x 8 clips per GPU" in j["config"]["workload"]
    assert j["config"]["prefill_batch_per_gpu"] == 16 and "replicated-prefill" in j["config"]["parallelism"]
    assert j["dist"]["world_size"] == 2 and j["dist"]["prefill"] == "replicated"
    sh = j["also"]["sharded_prefill"]
    assert sh["prefill_batch_per_gpu"] == 8 and sh["value"] > j["value"]          # (the replicated prefill does twice the LLM work)


def _gpu_count():
    try:
        import torch
        return torch.cuda.device_count()
    except Exception:
        return 0


needs_two_gpus = pytest.mark.skipif(_gpu_count() < 2, reason="needs >= 2 GPUs: RCCL over xGMI (the driver's 8-GPU node)")


@needs_two_gpus
def test_encode_clips_dp_over_rccl_bit_identical():
    """The same worker with one GPU per rank and the `nccl` backend (= RCCL on ROCm): the gathered pooled tokens of every case
    (equal / ragged / idle rank / frames mode) are bit-identical to the single-rank concat (SURVEY.md §8e "Verification").
    Skips itself on a 1-GPU box; runs by itself the day the suite lands on a multi-GPU node."""
    r = _run([os.path.join(ROOT, "tests", "dp_worker.py")], 2, 29651, extra_env={"VALLEY_DP_BACKEND": "nccl"})
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    for rank in range(2):
        assert f"DP_OK rank {rank}/2 backend nccl device {rank}" in r.stdout, r.stdout[-2000:]


@needs_two_gpus
def test_bench_two_gpus_over_rccl():
    """bench.py exactly as the driver launches it at N = 2 (c3, RCCL): the line says which backend carried the gather and what the
    gather cost — one pre-projection all-gather of 0.59 MB per clip is < 1 % of a step (SURVEY.md §8e "Collective")."""
    r = _run([os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--traffic", "none",
              "--also", "none"], 2, 29653, timeout=1200)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(line) == 1, r.stdout[-2000:]
    j = json.loads(line[0])
    d = j["dist"]
    assert j["n_gpus"] == 2 and d["world_size"] == 2 and d["rccl"] is True and d["backend"] == "nccl"
    assert d["allgather_share_of_step"] < 0.01, d
    assert d["vit_frames_per_s_all_gpus"] > 1.5 * d["vit_frames_per_s_per_gpu_min"]
