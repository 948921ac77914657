"""The two tails of c16_solve (sadvio_amd/csrc/chol16.h) give the same bits: tests/cpp/chol16_tail_check.hip, built here with the ROCm
compiler and run once.

The program includes the product header, factors seeded random SPD systems of N = 1 .. 174 (every size at which the last block
column or the back-substitution takes another path, or a block falls into the next wave) with the product's tail and with old_tail on the same image, and exits 0 only if
xs and the return value are equal bit for bit, the image of SOLVE = false is equal bit for bit, the solution agrees with a host
Cholesky solve, and a system with a non-positive pivot returns false from both. Its output is printed (run with -s)."""
import os
import shutil
import subprocess

import pytest

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu

SOURCE = os.path.join(ge.ROOT, "tests", "cpp", "chol16_tail_check.hip")
SIZES = (1, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 80, 112, 113, 114, 127, 128, 129, 165, 174)


def find_hipcc():
    return shutil.which("hipcc") or next((p for p in ("/opt/rocm/bin/hipcc",) if os.access(p, os.X_OK)), None)


def test_old_and_new_tail_give_the_same_bits(tmp_path):
    hipcc = find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc on this machine: tests/cpp/chol16_tail_check.hip was not built (profiles/r15_chol16_tail.txt holds a run made by hand)")
    exe = str(tmp_path / "chol16_tail_check")
    flags = [f for f in ge.HIP_FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.run([hipcc] + flags + ["-o", exe, SOURCE], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout + r.stderr)
    assert r.returncode == 0, r.stdout[-2000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "chol16_tail_check: OK"
    for n in SIZES:      # every size of the table was run and held
        assert any(ln.startswith(f"N={n:3d} returns 1 | 1, xs bit-equal, SOLVE=false image") and ln.endswith(" ok") for ln in lines), n
    assert any("non-positive pivot: new tail returns 0, old tail 0" in ln and ln.endswith(" ok") for ln in lines)
