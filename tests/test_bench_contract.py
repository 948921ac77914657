"""The driver reads ONE JSON line from bench.py's stdout. Libraries write to stdout as well (RCCL prints a banner through C stdio when a
communicator is created; buffered, it used to land after the record): bench.py claims fd 1 for the record alone."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stdout_carries_the_record_alone():
    code = (
        "import bench, ctypes\n"
        "emit = bench._claim_stdout()\n"
        "print('python noise')\n"
        "ctypes.CDLL(None).printf(b'buffered C noise before the record\\n')\n"
        "emit({'metric': 'x', 'value': 1.5})\n"
        "ctypes.CDLL(None).printf(b'C noise after the record\\n')\n"
    )
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 1 and json.loads(lines[0]) == {"metric": "x", "value": 1.5}
    for noise in ("python noise", "buffered C noise before the record", "C noise after the record"):
        assert noise in r.stderr


def test_bench_line_fields_of_the_committed_record():
    """profiles/r06_bench.json is a full line of the profiling box: the contract's fields, the roofline and the CPU baseline objects."""
    rec = json.load(open(os.path.join(ROOT, "profiles", "r06_bench.json")))
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
              "roofline", "cpu_baseline"):
        assert k in rec, k
    assert rec["dtype"] == "f64" and rec["vs_baseline"] is None and "workload" in rec["config"]
    assert rec["roofline"]["bound"] == "latency" and rec["batched"]["fp64"]["flops_per_lm_step_survey_8d"] == 470 * 40000 + 4100 * 8000 + 114 ** 3 // 3
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in rec["roofline"], k
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in rec["cpu_baseline"], k
    assert abs(rec["roofline"]["frac"] - rec["roofline"]["achieved"] / rec["roofline"]["peak"]) < 1e-4
    assert abs(rec["value"] - rec["config"]["solves_per_step"] * rec["config"]["iterations_per_solve"] / (rec["ms_per_step"] * 1e-3)) / rec["value"] < 1e-3


def test_gpus_n_without_n_gpus_refuses():
    """`bench.py --gpus 2` on a node without two GPUs fails with "needs 2 GPUs" - it never prints a one-rank record."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], capture_output=True, text=True, cwd=ROOT, timeout=300, env=env)
    import torch
    if torch.cuda.is_available() and torch.cuda.device_count() >= 2:
        return   # a multi-GPU box: the launch itself is covered by tests/test_gpu_multiprocess.py
    assert r.returncode != 0 and "needs 2 GPUs" in r.stderr and r.stdout.strip() == ""


def test_world_size_must_match_gpus():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"], capture_output=True, text=True, cwd=ROOT, timeout=300, env=env)
    assert r.returncode != 0 and "WORLD_SIZE = 2" in r.stderr and r.stdout.strip() == ""


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "0"], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode != 0 and "--steps must be >= 1" in r.stderr and r.stdout.strip() == ""


def test_full_is_off_by_default():
    import bench
    assert bench.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"]).full is False
    assert bench.parse_args(["--full"]).full is True


# what a --full run adds to the line; a plain run carries the contract's fields and `config` alone
FULL_ONLY = ("roofline", "cpu_baseline", "parity", "batched", "upload_inclusive", "marginalize", "backend_step", "vio_window", "sharded_window",
             "sharded_window_c5")


class _FakeBackend:
    """The part of capi.Backend that bench.dump_outputs reads: windows' sizes, get_deltas, get_ids."""

    def __init__(self, shapes):
        from types import SimpleNamespace
        self.windows = [SimpleNamespace(n_kf=k, n_lmk=n) for k, n in shapes]

    def get_deltas(self, w):
        import numpy as np
        k, n = self.windows[w].n_kf, self.windows[w].n_lmk
        rng = np.random.default_rng(w)
        return {"pose": rng.standard_normal((k, 6)), "lmk": rng.standard_normal((n, 3)), "dv": np.zeros((k, 3)), "dba": np.zeros((k, 3)),
                "dbg": np.zeros((k, 3))}

    def get_ids(self, w):
        import numpy as np
        return np.arange(self.windows[w].n_kf, dtype=np.int64) + 1000 * w, (np.int64(1) << 40) + np.arange(self.windows[w].n_lmk, dtype=np.int64)


def _summaries(n):
    from sadvio_amd import capi
    return [capi.SolveSummary(iterations=10, num_successful_steps=9, num_unsuccessful_steps=1, termination=0, initial_cost=5.0 + w,
                              final_cost=1.0 + w, fixed_cost=0.0, final_radius=1e4) for w in range(n)]


def test_dump_outputs_writes_every_window_in_float64(tmp_path):
    import numpy as np
    import bench
    be = _FakeBackend([(20, 800), (5, 40), (12, 300)])
    total = bench.dump_outputs(str(tmp_path), be, _summaries(3))
    files = sorted(os.listdir(tmp_path))
    assert total == sum(os.path.getsize(tmp_path / f) for f in files)
    arrays = {f[:-4]: np.load(tmp_path / f) for f in files}
    assert all(a.dtype == np.float64 for a in arrays.values())
    assert arrays["windows"].tolist() == [0, 1, 2]
    assert arrays["summary"].shape == (3, 8) and arrays["summary"][:, 0].tolist() == [10, 10, 10] and arrays["summary"][:, 5].tolist() == [1, 2, 3]
    for w in range(3):
        d = be.get_deltas(w)
        kf_id, lmk_id = be.get_ids(w)
        for k in ("pose", "lmk", "dv", "dba", "dbg"):
            assert np.array_equal(arrays[f"w{w}_{k}"], d[k])
        assert np.array_equal(arrays[f"w{w}_kf_id"].astype(np.int64), kf_id) and np.array_equal(arrays[f"w{w}_lmk_id"].astype(np.int64), lmk_id)


def test_dump_outputs_samples_windows_within_the_budget(tmp_path):
    import numpy as np
    import bench
    be = _FakeBackend([(20, 8000)] * 40)
    budget = 2 << 20    # ~8 of the 40 windows
    total = bench.dump_outputs(str(tmp_path / "a"), be, _summaries(40), budget=budget)
    assert total <= budget
    kept = np.load(tmp_path / "a" / "windows.npy").astype(int).tolist()
    assert 0 < len(kept) < 40 and kept == sorted(kept)
    assert sorted(f for f in os.listdir(tmp_path / "a") if f.endswith("_lmk.npy")) == sorted(f"w{w}_lmk.npy" for w in kept)
    bench.dump_outputs(str(tmp_path / "b"), be, _summaries(40), budget=budget)
    assert np.load(tmp_path / "b" / "windows.npy").astype(int).tolist() == kept     # a fixed, seeded sample


@pytest.mark.gpu
def test_bench_dump_outputs_of_the_timed_path(tmp_path):
    """bench.py --dump-outputs on the GPU: the record's steps / ms_per_step, and the dumped deltas and ids are the timed window's
    (a fresh solve of the same seeded window in this process)."""
    import numpy as np
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--solves-per-step", "2", "--batch", "0",
           "--no-cpu-baseline", "--no-marginalize", "--no-sharded", "--no-vio", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert rec["steps"] == 3 and rec["ms_per_step"] > 0 and rec["config"]["solves_per_step"] == 2
    files = os.listdir(out)
    assert sum(os.path.getsize(out / f) for f in files) <= 64 << 20
    arrays = {f[:-4]: np.load(out / f) for f in files}
    assert all(a.dtype == np.float64 for a in arrays.values())
    assert arrays["windows"].tolist() == [0] and arrays["summary"].shape == (1, 8)
    import bench
    from sadvio_amd import capi, synthetic
    w = synthetic.make_window(seed=20250404)
    be = capi.Backend(device=0, use_graph=True)
    try:
        be.set_windows([w])
        s = be.solve(capi.gn_options(bench.GN_ITERS))[0]
        d = be.get_deltas(0)
    finally:
        be.close()
    assert int(arrays["summary"][0, 0]) == s.iterations == bench.GN_ITERS
    assert abs(arrays["summary"][0, 5] - s.final_cost) <= 1e-9 * abs(s.final_cost)
    assert np.array_equal(arrays["w0_kf_id"].astype(np.int64), w.kf_id) and np.array_equal(arrays["w0_lmk_id"].astype(np.int64), w.lmk_id)
    assert np.abs(arrays["w0_pose"] - d["pose"]).max() <= 1e-9 and np.abs(arrays["w0_lmk"] - d["lmk"]).max() <= 1e-8


@pytest.mark.gpu
def test_plain_run_carries_the_headline_alone():
    """A plain run times the steps and prints the contract's fields: no other leg runs, none of their objects is in the line."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--solves-per-step", "5"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1
    rec = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "ms_per_solve", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config"):
        assert k in rec, k
    assert not [k for k in FULL_ONLY if k in rec]
    assert rec["steps"] == 2 and rec["warmup"] == 1 and rec["dtype"] == "f64" and rec["higher_is_better"] is True
    assert rec["config"]["solves_per_step"] == 5 and rec["config"]["iterations_per_solve"] == 10
    assert abs(rec["value"] - 5 * 10 / (rec["ms_per_step"] * 1e-3)) / rec["value"] < 1e-3


@pytest.mark.gpu
def test_full_run_adds_the_selected_legs():
    """--full with the slow legs switched off: the roofline's profiled pass and the upload-inclusive rate are in the line, the
    legs its options skip are null."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--solves-per-step", "5", "--full",
           "--batch", "0", "--no-cpu-baseline", "--no-marginalize", "--no-sharded", "--no-vio"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert set(FULL_ONLY) <= set(rec)
    assert rec["roofline"]["kernel"] in rec["roofline"]["kernels_us"] and rec["upload_inclusive"]["value"] > 0
    assert rec["upload_inclusive"]["two_handles"]["value"] > 0
    for k in ("cpu_baseline", "parity", "batched", "marginalize", "backend_step", "vio_window", "sharded_window", "sharded_window_c5"):
        assert rec[k] is None, k
