"""HipOptimizer::set_device_model_gate (include/sadvio_optimizer.hpp). CPU: tests/cpp/test_model_gate.cpp compiles with g++ -std=c++17
-Wall -Werror against include/ and links the library (sadvio_ba_landmark_chi2_models must be exported); GPU: the program runs
landmarkOptimization on a double-sphere map with the chi2 gate on the device and on the host and requires identical outlier flags and
landmark positions, on the solved window and on the re-uploaded all-features window."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_model_gate.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "test_model_gate")


def build():
    import __graft_entry__ as g
    g.build_hip()
    lib_dir = os.path.join(ROOT, "sadvio_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), SRC, "-L", lib_dir, "-lsadvio_ba",
           "-Wl,-rpath," + lib_dir, "-o", BIN]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return BIN


def test_cpp_model_gate_compiles_and_links():
    assert os.path.exists(build())


@pytest.mark.gpu
def test_device_gate_equals_host_gate_in_landmark_optimization():
    r = subprocess.run([build()], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASSED" in r.stdout
