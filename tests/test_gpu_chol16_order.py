"""The instruction order of c16_solve (sadvio_amd/csrc/chol16.h) does not change a bit: tests/cpp/chol16_order_check.hip, built here
twice with the ROCm compiler — as the product has it, and with -DSADVIO_C16_PARENT_ORDER (the back-substitution in the order it had
before the H column of a step was requested one step ahead) — and each build run once.

Each build factors the seeded random SPD systems of tests/cpp/chol16_tail_check.hip (N = 1 .. 174: every size at which the last block
column or the back-substitution takes another path, or a block falls into the next wave, and one system with a non-positive pivot)
with both tails and writes xs, the return values and the whole image of SOLVE = false to a file. The two files must be equal byte
for byte. Each build also holds the solution against a host Cholesky solve and returns false on the non-positive pivot, or it does not
exit with 0. The programs' output is printed (run with -s)."""
import os
import shutil
import subprocess

import pytest

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu

SOURCE = os.path.join(ge.ROOT, "tests", "cpp", "chol16_order_check.hip")
MACRO = "-DSADVIO_C16_PARENT_ORDER"
SIZES = (1, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 80, 112, 113, 114, 127, 128, 129, 165, 174)


def find_hipcc():
    return shutil.which("hipcc") or next((p for p in ("/opt/rocm/bin/hipcc",) if os.access(p, os.X_OK)), None)


def expected_bytes():
    """Size of a build's file: per size and tail  N, old_tail, return value, xs[N], return value, image."""
    blocks = lambda n: (n + 15) // 16
    image = lambda n: blocks(n + 1) * (blocks(n + 1) + 1) // 2 * 256
    return sum(2 * (16 + 8 * n + 8 * image(n)) for n in SIZES + (114,))


def test_parent_order_and_product_order_give_the_same_bytes(tmp_path):
    hipcc = find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc on this machine: tests/cpp/chol16_order_check.hip was not built (profiles/r17_solve_chain.txt holds a run made by hand)")
    flags = [f for f in ge.HIP_FLAGS if f not in ("-shared", "-fPIC")]
    builds = {"product": [], "parent": [MACRO]}
    exe = {k: str(tmp_path / f"chol16_order_check_{k}") for k in builds}
    procs = {k: subprocess.Popen([hipcc] + flags + extra + ["-o", exe[k], SOURCE]) for k, extra in builds.items()}   # the two compilations side by side
    for k, p in procs.items():
        assert p.wait(timeout=600) == 0, f"build of the {k} order failed"
    data = {}
    for k in builds:
        out = str(tmp_path / f"{k}.bin")
        r = subprocess.run([exe[k], out], capture_output=True, text=True, timeout=120)
        print(r.stdout + r.stderr)
        assert r.returncode == 0, r.stdout[-2000:]
        lines = r.stdout.splitlines()
        assert lines[-1] == f"chol16_order_check: OK ({k} order)"
        for n in SIZES:      # every size of the table was run with both tails and held against the host solve
            for tail in (0, 1):
                assert any(ln.startswith(f"N={n:3d} old_tail {tail} returns 1 | 1,") and ln.endswith(" ok") for ln in lines), (k, n, tail)
        assert sum("non-positive pivot" in ln and "returns 0" in ln and ln.endswith(" ok") for ln in lines) == 2, k
        with open(out, "rb") as f:
            data[k] = f.read()
        assert len(data[k]) == expected_bytes(), (k, len(data[k]), expected_bytes())
    assert data["product"] == data["parent"], "xs, a return value or an image of SOLVE = false differs between the two orders"
