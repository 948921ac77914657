"""The sharded-window protocol across REAL processes: two / three processes launched by
torch.distributed.run, each owning a handle on the box's one GPU, the per-LM-step all-reduce of the reduced system going
through sadvio_ba_set_collective into torch.distributed (gloo). This drives the library's rank logic exactly as an
8-GPU node would (there the hook is the built-in RCCL one, sadvio_ba_comm_init_rccl): different address spaces, no
shared Python state, a collective that really crosses process boundaries."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_window_across_processes(tmp_path, world):
    out = tmp_path / "record.json"
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "mp_sharded_worker.py"), str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rec = json.load(open(out))
    a = rec["lds"]
    assert a["iterations"] == [a["single_iterations"]] * world == [a["oracle_iterations"]] * world
    assert a["termination"] == [a["single_termination"]] * world
    assert a["pose_identical_across_ranks"]
    assert a["dpose_vs_oracle"] <= 1e-6 and a["dlmk_vs_oracle"] <= 1e-5 and a["dpose_vs_single"] <= 1e-9
    assert a["allreduce_calls"] >= 2 * a["single_iterations"] - 1       # two collectives per executed LM step
    b = rec["banded_hbm"]
    assert b["pose_identical_across_ranks"] and b["dpose_vs_single"] <= 1e-6 and b["dlmk_vs_single"] <= 1e-5 and b["dcost_rel"] <= 1e-9
    assert b["max_count"] < b["n_p"] * b["n_p"] // 2                    # only the band of the reduced system travels


def _gpu_count():
    import torch
    return torch.cuda.device_count() if torch.cuda.is_available() else 0


@pytest.mark.skipif(_gpu_count() < 2, reason="needs two physical GPUs: the built-in RCCL all-reduce across devices (VERDICT r05 item 2)")
def test_sharded_window_over_rccl_on_two_gpus(tmp_path):
    """One rank per GPU, ncclCommInitRank over xGMI, the reduced system all-reduced by RCCL itself: the first box with two GPUs that
    runs this suite exercises N > 1 without a code change. Same bars as the gloo-backed case: oracle, single-device solve, bit-identical
    poses on every rank."""
    out = tmp_path / "record.json"
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "mp_sharded_worker.py"), str(out), "rccl"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rec = json.load(open(out))
    a, b = rec["lds"], rec["banded_hbm"]
    assert a["rccl"] and a["iterations"] == [a["single_iterations"]] * 2 == [a["oracle_iterations"]] * 2
    assert a["pose_identical_across_ranks"] and a["dpose_vs_oracle"] <= 1e-6 and a["dlmk_vs_oracle"] <= 1e-5 and a["dpose_vs_single"] <= 1e-9
    assert b["pose_identical_across_ranks"] and b["dpose_vs_single"] <= 1e-6 and b["dlmk_vs_single"] <= 1e-5 and b["dcost_rel"] <= 1e-9


def test_bench_gpus_2_runs_two_ranks_or_refuses(tmp_path):
    """`python bench.py --gpus 2` with no launcher around it: on a node with two GPUs it re-execs through torch.distributed.run and the
    record says n_gpus = 2 with a two-rank RCCL communicator; on this pool's one-GPU box it must REFUSE (never a one-rank record)."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("WORLD_SIZE", None); env.pop("RANK", None); env.pop("LOCAL_RANK", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--solves-per-step", "20",
                        "--full", "--no-cpu-baseline"], capture_output=True, text=True, timeout=1500, env=env, cwd=ROOT)
    if _gpu_count() < 2:
        assert r.returncode != 0 and "needs 2 GPUs" in r.stderr and r.stdout.strip() == ""
        return
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert rec["n_gpus"] == 2 and rec["sharded_window"]["config"]["rccl_ranks"] == 2 and rec["sharded_window_c5"] is not None
