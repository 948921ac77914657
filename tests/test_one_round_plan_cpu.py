"""LayoutPlan::single_round, the layout's half of the gate of the single-round tile kernels: tests/cpp/test_one_round_plan.cpp, plain g++,
no GPU; once as it stands and once as a stand-alone host program under AddressSanitizer and UBSan."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "asan_ubsan"])
def test_single_round_plan(tmp_path, flags):
    exe = str(tmp_path / "test_one_round_plan")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags + [os.path.join(ROOT, "tests", "cpp", "test_one_round_plan.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "PASSED" in r.stdout, r.stdout + r.stderr
