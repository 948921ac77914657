"""Every window of the tile-kernel cases of tests/step_helpers.py reaches the variant it is meant to reach: the host-only planner
(sadvio_amd/csrc/layout_plan.h, through tests/cpp/dump_tile_plan.cpp: plain g++, no GPU) is given the window's track structure and
the case's switches, and its tiles (mode, lanes per landmark, landmarks, free key-frames, packed or contiguous), its chunks and its
plan-wide flags must be the ones the case records. A GPU test cannot see a tile's mode; this one can. The builder conditions of
the cases are asserted here as well."""
import os
import subprocess

import numpy as np
import pytest

import step_helpers as sh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dump_tile_plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tile_plan") / "dump_tile_plan")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "dump_tile_plan.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(ws, env):
        p = subprocess.run([exe], input=sh.plan_input(ws, env), capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        return sh.parse_plan(p.stdout)
    return run


@pytest.mark.parametrize("case", sh.TILE_CASES, ids=[c.name for c in sh.TILE_CASES])
def test_planner_puts_the_case_where_its_table_says(dump_tile_plan, case):
    ws = sh.case_windows(case)
    plan = dump_tile_plan(ws, case.env)
    want = case.plan
    mine = [t for t in plan["tiles"] if t["w"] == len(ws) - 1]
    assert [(t["lds_mode"], t["G"], t["n_lmk"], t["n_free"]) for t in mine] == want["tiles"], mine
    assert all(t["packed"] == want["packed"] for t in mine), mine
    assert sum(t["n_lmk"] for t in mine) == ws[-1].n_lmk
    for k in ("lm_ok", "lm_ksub", "lm_n_sub", "pre_ok"):
        assert plan[k] == want[k], (k, plan[k], want[k])
    assert plan["gemm_run4"] == 0                        # (RARE is reached through the loss, never through runs of 3 - 4 observations)
    if want["chunks"] is not None:
        assert [t["chunks"] for t in mine] == want["chunks"], [t["chunks"] for t in mine]
    else:
        assert all(t["chunks"] == [] for t in mine)
    if case.kernels == "throughput":                     # the whole batch, decoys included, must be chunked MFMA tiles
        assert all(t["lds_mode"] == 2 for t in plan["tiles"])


def test_chunk_cuts_restates_the_planner_on_the_mixed_window(dump_tile_plan):
    """lm_mixed has a chunk closed by the 64-observation limit and one closed by the 12-landmark limit (and chunk_cuts, which says
    so, cuts as the planner does)."""
    case = sh.CASE["lm_mixed"]
    w = sh.case_window(case)
    counts = np.diff(w.lmk_obs_ptr).tolist()
    assert counts == list(sh.LM_MIXED_COUNTS) and min(counts) == 2 and max(counts) == 8
    cuts = sh.chunk_cuts(counts)
    plan = dump_tile_plan([w], case.env)
    assert [(a, b) for a, b, _ in cuts] == [c for t in plan["tiles"] for c in t["chunks"]]
    closed = {why for _, _, why in cuts}
    assert "obs" in closed and "lmk" in closed
    assert any(why == "obs" and no < 64 for _, no, why in cuts)       # cut by the NEXT landmark, not by a full wave


@pytest.mark.parametrize("window", ["w70_huber"])
def test_huber_window_has_residuals_on_both_sides_of_the_threshold(window):
    case = sh.CASE[window]
    assert case.opts["huber_a"] == sh.HUBER_A
    share = sh.beyond_huber(sh.case_window(case))
    print(f"{window}: {100 * share:.0f} % of the observations beyond the Huber threshold at x = 0")
    assert 0.1 <= share <= 0.9


def test_cases_of_one_window_share_its_options_and_size():
    by_window = {}
    for c in sh.CASES:
        first = by_window.setdefault(c.window, c)
        assert (first.opts, first.np_, first.golden) == (c.opts, c.np_, c.golden), (first.name, c.name)
    for c in sh.TILE_CASES:
        w = sh.case_window(c)
        assert sh.reduced_np(w) == c.np_ <= sh.MAX_LDS_NP and len(w.obs_kf) <= 350, c.name
        assert sh.free_kf_observations(w).min() >= 10, c.name
