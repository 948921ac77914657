"""The headers taken out of kernels.h, and the headers that use them, compile on their own: a translation unit that consists of
one #include of the header passes hipcc -fsyntax-only for gfx950, with and without the in-kernel timestamps (-DSADVIO_KERNEL_TS). A header that leans on what another
one happened to include in front of it fails here, not in whoever reorders the includes next. No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sadvio_amd", "csrc")
# the headers taken out of kernels.h, kernels.h itself, the headers that call the helpers they share, and chol16.h
HEADERS = ["step_args.h", "wave_ops.h", "tile_common.h", "kernels.h", "chol16.h", "dense_chol.h", "long_kernels.h", "ba_handle.h"]


@pytest.mark.parametrize("header", HEADERS)
def test_header_compiles_alone(header, tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = tmp_path / "unit.hip"
    src.write_text(f'#include "{header}"\n')
    for extra in ([], ["-DSADVIO_KERNEL_TS"]):
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", "-I", CSRC] + extra + [str(src)],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, f"{header} {' '.join(extra)}\n{r.stderr[-4000:]}"
