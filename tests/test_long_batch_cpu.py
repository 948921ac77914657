"""CPU side of SADVIO_CFG_LONG_TRACK_BATCH (sadvio_ba_covariance_batch and the relative marginalisations on windows with long
tracks): the two host-only headers as stand-alone programs, the flag in the header and in both bindings. No GPU.

  tests/cpp/test_rel_runs.cpp        sadvio_amd/csrc/rel_runs.h: the bisection against the linear walk; built once more with
                                     -DPLANT_SHORT_RUN, whose off-by-one the program has to report.
  tests/cpp/test_covb_long_plan.cpp  sadvio_amd/csrc/covb_long_plan.h: the work table of one group of units.
Both also run under the address and undefined-behaviour sanitizers (host code only; nothing of it is loaded into Python or run on a
GPU)."""
import inspect
import os
import re
import subprocess

import pytest

from sadvio_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]


def _build_and_run(tmp_path, source, name, extra=()):
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, os.path.join(ROOT, "tests", "cpp", source), "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], capture_output=True, text=True)


@pytest.mark.parametrize("sanitize", [False, True])
def test_bisection_visits_what_the_walk_visits(tmp_path, sanitize):
    r = _build_and_run(tmp_path, "test_rel_runs.cpp", "rel_runs", SANITIZE if sanitize else ())
    print(r.stdout.strip().splitlines()[-2])
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr


def test_a_planted_short_run_shows(tmp_path):
    r = _build_and_run(tmp_path, "test_rel_runs.cpp", "rel_runs_planted", ["-DPLANT_SHORT_RUN"])
    print(r.stdout.strip().splitlines()[-1])
    assert r.returncode == 1 and "MISMATCH" in r.stdout and not r.stdout.strip().endswith("OK"), r.stdout + r.stderr


@pytest.mark.parametrize("sanitize", [False, True])
def test_group_work_table(tmp_path, sanitize):
    r = _build_and_run(tmp_path, "test_covb_long_plan.cpp", "covb_long_plan", SANITIZE if sanitize else ())
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr


def test_flag_matches_the_header_and_the_bindings_take_it(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "sadvio_ba.h")).read()
    m = re.search(r"#define\s+SADVIO_CFG_LONG_TRACK_BATCH\s+(\d+)", hdr)
    assert m and int(m.group(1)) == capi.CFG_LONG_TRACK_BATCH == 8
    p = inspect.signature(capi.Backend.__init__).parameters
    assert "long_track_batch" in p and p["long_track_batch"].default is False
    src = tmp_path / "long_batch.cpp"
    src.write_text('#include "sadvio_optimizer.hpp"\n'
                   'static_assert(SADVIO_CFG_LONG_TRACK_BATCH == 8 && (SADVIO_CFG_LONG_TRACKS | SADVIO_CFG_LONG_TRACK_PRIORS | '
                   'SADVIO_CFG_LONG_TRACK_COVARIANCE | SADVIO_CFG_LONG_TRACK_BATCH) == 15, "flags");\n'
                   "void make() { sadvio::HipOptimizer a(0, false, true, false, false, true); sadvio::HipOptimizer b(0, false, true, true, true, true); (void)a; (void)b; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
