"""CPU checks behind tests/test_gpu_long_tracks.py (no GPU):
  - the E_REF table of tests/long_track_helpers.py brackets the oracle's measured float64 error against the 50-digit step on every
    window, the oracle accepts that step, and its trace row carries the 50-digit model cost change and cost;
  - the committed 50-digit fixture equals a fresh computation (on the cheapest window);
  - the windows are what their names say (observation counts, rounds, the invalid observation in the second round, residuals on
    both sides of the Huber corner, a reduced system out of LDS whose band the long track fills);
  - a planted defect on the oracle: with ONE observation of a long track dropped (the 65th of its sorted list, or the first) the
    step moves by far more than the bar of the GPU test, so the bar sees a forgotten round or a forgotten lane."""
import numpy as np
import pytest

import long_track_helpers as lh
import step_helpers as sh
from sadvio_amd import capi

mp = pytest.importorskip("mpmath")


@pytest.mark.parametrize("case", lh.CASES, ids=[c.name for c in lh.CASES])
def test_e_ref_table_brackets_the_measured_values(oracle_lib, case):
    w = lh.case_window(case)
    f64 = sh.oracle_step(oracle_lib, w, lh.case_options(case))
    ref = lh.reference(case)
    e = sh.step_error(f64, ref, w)
    print(f'E_REF "{case.window}": ({e[0]:.2e}, {e[1]:.2e}),')
    for part, m, t in zip(("pose", "landmark"), e, lh.E_REF[case.window]):
        assert m <= t <= 4.0 * m, (part, m, t)
    assert np.isclose(f64["log"][1][7], ref["model_cost_change"], rtol=1e-11)
    assert np.isclose(f64["log"][1][0], ref["cost"], rtol=1e-11)


def test_fixture_equals_a_fresh_50_digit_step(oracle_lib):
    case = lh.CASE["L65_angular"]
    fresh, stored = lh.reference(case, oracle_lib, fresh=True), lh.reference(case)
    for k in ("pose", "lmk", "dv", "dba", "dbg"):
        assert np.array_equal(fresh[k], stored[k]), k
    assert fresh["model_cost_change"] == stored["model_cost_change"] and fresh["cost"] == stored["cost"]


def test_windows_are_what_their_names_say(oracle_lib):
    n = {c.name: lh.counts(lh.case_window(c)) for c in lh.CASES}
    assert set(n["L65"]) == {65} and len(n["L65"]) == 12 and set(n["L128"]) == {128} and set(n["L129"]) == {129} and len(n["L129"]) == 6
    assert sorted(n["MIX"])[-3:] == [66, 68, 70] and (n["MIX"] == 5).sum() == 60
    mix = lh.case_window(lh.CASE["MIX"])
    assert mix.lmk_const[31] == 1 and n["MIX"][31] == 70 and mix.kf_const.sum() == 34
    for l in lh.long_landmarks(mix):                                  # constant and free observers of every long track
        kc = mix.kf_const[mix.obs_kf[mix.lmk_obs_ptr[l]:mix.lmk_obs_ptr[l + 1]]]
        assert (kc == 1).any() and (kc == 0).any()
    vio = lh.case_window(lh.CASE["VIO"])
    assert vio.has_imu == 1 and len(vio.imu_factors) == vio.n_kf - 1 and n["VIO"].max() == 66 and sh.layout(vio)["dpf"] == 15
    share = sh.beyond_huber(lh.case_window(lh.CASE["L65_huber"]))
    assert 0.1 <= share <= 0.9, share
    # the invalid observation: exactly one, at position 64 of its landmark's key-frame-sorted list
    inv = lh.case_window(lh.CASE["L65_invalid"])
    valid = oracle_lib.linearize(inv)[3]
    bad = np.flatnonzero(np.asarray(valid) == 0)
    assert bad.tolist() == [lh.second_round_observation(inv, lh.INVALID_LMK)]
    assert np.asarray(oracle_lib.linearize(lh.case_window(lh.CASE["L65"]))[3]).all()
    big = lh.case_window(lh.CASE["BIG"])
    lay = sh.layout(big)
    assert lay["Nr"] == 240 > sh.MAX_LDS_NP and sh.band_rows(big) == 240 and sh.expected_route(240, 6, 240) == "wide"
    assert sh.free_kf_observations(big).min() >= 10


@pytest.mark.parametrize("which", ["the 65th", "the first"])
def test_one_dropped_observation_lands_far_above_the_bar(oracle_lib, which):
    import test_gpu_tile_packing as tp
    case = lh.CASE["L65"]
    w = lh.case_window(case)
    l = 5
    o = np.arange(w.lmk_obs_ptr[l], w.lmk_obs_ptr[l + 1])
    order = np.argsort(w.obs_kf[o], kind="stable")                    # the device's order
    drop = order[64] if which == "the 65th" else order[0]
    keep = np.setdiff1d(np.arange(65), [drop])
    d = tp._assemble(w, [(w, q, keep if q == l else None) for q in range(w.n_lmk)])
    d.kf_id, d.lmk_id = w.kf_id, w.lmk_id
    got = sh.oracle_step(oracle_lib, d, lh.case_options(case))
    e = sh.step_error(got, lh.reference(case), w)
    bar_p, bar_l = lh.bars(case)
    print(f"L65 without {which} observation of landmark {l}: pose {e[0]:.1e} ({e[0] / bar_p:.1e} x bar) landmark {e[1]:.1e} ({e[1] / bar_l:.1e} x bar)")
    assert e[0] > 1e3 * bar_p or e[1] > 1e3 * bar_l
