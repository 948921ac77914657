"""HipOptimizer::landmarkOptimizationNoFov (include/sadvio_optimizer.hpp). CPU: tests/cpp/test_nofov.cpp compiles and links
against include/ and the library, and tests/cpp/test_nofov_flatten.cpp checks the landmark selection with no device; GPU: the
program runs the solve on the scaleTest rig and checks the write-back rules."""
import os
import subprocess

import numpy as np
import pytest

import nofov_helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_nofov.cpp")


def build(tmp_path):
    import __graft_entry__ as g
    g.build_hip()
    lib_dir = os.path.join(ROOT, "sadvio_amd", "csrc")
    exe = str(tmp_path / "test_nofov")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), SRC, "-L", lib_dir, "-lsadvio_ba",
           "-Wl,-rpath," + lib_dir, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def rig_args():
    fx = H.fixture()
    return [repr(float(v)) for k in ("T_f_s1", "T_f_s2", "T_f_fp") for v in np.asarray(fx[k]).ravel()]


def test_nofov_host_layer_compiles_and_links(tmp_path):
    assert os.path.exists(build(tmp_path))


def test_nofov_flatten_selection_rules(tmp_path):
    exe = str(tmp_path / "test_nofov_flatten")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "test_nofov_flatten.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "PASSED" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_nofov_host_layer_write_back(tmp_path):
    r = subprocess.run([build(tmp_path)] + rig_args(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASSED" in r.stdout
