"""HipOptimizer's fifth constructor argument, long_track_covariance (include/sadvio_optimizer.hpp): a translation unit that names it
compiles with the host compiler (-fsyntax-only, -Wall -Werror); the flag it sets is the header's. No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SOURCE = """#include "sadvio_optimizer.hpp"
static_assert(SADVIO_CFG_LONG_TRACK_COVARIANCE == 4 && (SADVIO_CFG_LONG_TRACKS | SADVIO_CFG_LONG_TRACK_PRIORS | SADVIO_CFG_LONG_TRACK_COVARIANCE) == 7, "flags");
void make() { sadvio::HipOptimizer a(0, false, true, false, true); sadvio::HipOptimizer b(0, false, true, true, true); (void)a; (void)b; }
"""


def test_five_argument_constructor_compiles(tmp_path):
    src = tmp_path / "long_cov.cpp"
    src.write_text(SOURCE)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
