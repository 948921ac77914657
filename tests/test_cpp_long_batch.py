"""HipOptimizer's sixth constructor argument, long_track_batch (include/sadvio_optimizer.hpp). CPU: tests/cpp/test_long_batch.cpp
compiles with -Wall -Werror and links against include/ and the library; GPU: marginalizeRelativeBatch on a snapshot with a
68-observation landmark returns true on such an optimizer and is refused, with the long-track text, on one with long_tracks alone."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_long_batch.cpp")


def build(tmp_path):
    import __graft_entry__ as g
    g.build_hip()
    lib_dir = os.path.join(ROOT, "sadvio_amd", "csrc")
    exe = str(tmp_path / "test_long_batch")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), SRC, "-L", lib_dir, "-lsadvio_ba",
           "-Wl,-rpath," + lib_dir, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_long_batch_host_layer_compiles_and_links(tmp_path):
    assert os.path.exists(build(tmp_path))


@pytest.mark.gpu
def test_long_batch_host_layer_serves_a_snapshot_with_a_long_track(tmp_path):
    r = subprocess.run([build(tmp_path)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASSED" in r.stdout
