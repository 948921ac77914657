"""HipOptimizer::covarianceCross and innovation_gate (include/sadvio_optimizer.hpp) from C++. CPU: tests/cpp/test_covariance_cross.cpp
compiles with -Wall -Werror and links against include/ and the library (sadvio_ba_covariance_cross must be exported); GPU: the
program solves a small local map and checks addressing by id, the joint covariance of every candidate, the gate and the refusals."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_covariance_cross.cpp")


def build(tmp_path):
    import __graft_entry__ as g
    g.build_hip()
    lib_dir = os.path.join(ROOT, "sadvio_amd", "csrc")
    exe = str(tmp_path / "test_covariance_cross")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), SRC, "-L", lib_dir, "-lsadvio_ba",
           "-Wl,-rpath," + lib_dir, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_covariance_cross_program_compiles_and_links(tmp_path):
    assert os.path.exists(build(tmp_path))


@pytest.mark.gpu
def test_covariance_cross_program(tmp_path):
    r = subprocess.run([build(tmp_path)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASSED" in r.stdout
