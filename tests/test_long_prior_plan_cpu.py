"""The host-only planner (sadvio_amd/csrc/layout_plan.h) with long tracks held in the reduced system by priors, through
tests/cpp/dump_long_prior_plan.cpp (plain g++, no GPU). For KMIX (tests/long_prior_helpers.py) under the prior of its marginalisation:
  - the three kept long tracks are on the long list AND on the kept list with all 66 observations each, lmk_const_red = 2;
  - N_p = 6 n_free + 3 x 6, and the kept short tracks are on the kept list with their 5 observations;
  - a pose-to-landmark factor on a free long track holds it (a listed factor, 3 more columns) and appends no pseudo-observation, while
    the same factor on a short track rides the elimination as two pseudo-observations, as it always did;
  - without LayoutIn::long_priors (a handle created without SADVIO_CFG_LONG_TRACK_PRIORS) the same plans are refused with the texts
    they always had.
That windows without long tracks plan as before long tracks existed is held by tests/test_long_plan_cpu.py
(tests/golden/plan_dump_before_long_tracks.txt), which runs unchanged."""
import subprocess

import pytest

import long_prior_helpers as ph
import long_track_helpers as lh
import step_helpers as sh
from test_long_plan_cpu import _compile


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = _compile(tmp_path_factory.mktemp("long_prior_plan"), "dump_long_prior_plan")

    def run(w, keep=(), p2l=(), long_priors=1, long_min=65):
        tail = " ".join(str(int(v)) for v in [len(keep), *keep, len(p2l), *[x for f in p2l for x in f]])
        p = subprocess.run([exe], input=f"{long_min} {long_priors}\n" + sh.plan_input([w], {}) + tail + "\n", capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        out = {"L": [], "K": [], "S": [], "error": None}
        for line in p.stdout.splitlines():
            v = line[2:].split()
            if line[0] == "E":
                out["error"] = line[2:]
            elif line[0] in "PW":
                out[line[0]] = [int(x) for x in v]
            else:
                out[line[0]].append([int(x) for x in v])
        return out
    return run


def test_kmix_under_its_prior(dump):
    w = ph.case_window(ph.CASE["KMIX"])
    keep = ph.marg_args(w)["lmk_keep"]
    long_ = lh.long_landmarks(w).tolist()
    kept_long = [l for l in keep if l in long_]
    n_free = int((w.kf_const == 0).sum())
    plan = dump(w, keep=keep)
    assert plan["error"] is None, plan["error"]
    assert plan["P"] == [4, 3 * 66 + 3 * 5]                           # every long track on the long list | the kept list: every observation of the six
    assert plan["W"] == [0, 6 * n_free + 3 * 6, 6, w.n_obs, w.n_obs]  # no pseudo-observation
    col = {l: 6 * n_free + 3 * i for i, l in enumerate(keep)}
    for _, _, l, n_obs, on_list, code, red in plan["L"]:
        assert n_obs == 66
        assert (on_list, code, red) == ((66, 2, col[l]) if l in kept_long else (0, 0, -1)), l
    assert [r[2] for r in plan["L"]] == long_
    assert sorted(r[1] for r in plan["K"]) == [l for l in keep if l not in long_]
    for _, l, on_list, code, red in plan["K"]:
        assert (on_list, code, red) == (5, 2, col[l])
    refused = dump(w, keep=keep, long_priors=0)
    assert refused["error"] == "long tracks: a prior factor keeps or touches a landmark on the long path"
    assert dump(w, keep=[l for l in keep if l not in long_], long_priors=0)["error"] is None      # short tracks: kept as always


def test_a_pose_to_landmark_factor_holds_a_long_track_and_rides_a_short_one(dump):
    w = ph.case_window(ph.CASE["KMIX"])
    n_free = int((w.kf_const == 0).sum())
    free_long, short = 61, 5
    plan = dump(w, p2l=[(0, free_long), (0, short)])
    assert plan["error"] is None, plan["error"]
    assert plan["W"] == [0, 6 * n_free + 3, 1, w.n_obs + 2, w.n_obs]  # the short track's two pseudo-observations only
    assert plan["S"] == [[0, 0, 1, free_long], [0, 1, 4, short]]      # listed (SADVIO_SPARSE_POSE_TO_LMK) | rides the elimination (internal type 4)
    row = [r for r in plan["L"] if r[2] == free_long][0]
    assert row[3:] == [66, 66, 2, 6 * n_free]
    assert plan["K"] == []
    e = dump(w, p2l=[(0, free_long)], long_priors=0)["error"]
    assert e == "long tracks: a pose-to-landmark factor of the sparse prior touches a landmark on the long path"
