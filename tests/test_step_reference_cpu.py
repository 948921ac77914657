"""The 50-digit first LM step of tests/step_helpers.py, checked without a GPU:
  - against the twin's independent un-reduced 50-digit solve (oracle/twin.py) on two tiny windows;
  - the E_REF table of the helper brackets the oracle's measured float64 error on every window of tests/test_gpu_first_step.py;
  - a float64 host model of the blocked in-LDS Cholesky solve with a planted defect lands ABOVE the bar of the GPU test in every
    in-LDS case: the bar is tight enough to see an unrefined reciprocal-square-root seed on one pivot, a dropped rank-4 product on one
    tile and a column whose damping is missing; the same model without a defect passes the bar;
  - a float64 host model of the TILE kernels (the un-reduced system summed observation by observation from the twin's Jacobian
    rows) stays within both bars on every window of the tile-kernel cases, and lands above the bar with one observation scaled by
    1 + 2^-24, one landmark pivot's unrefined reciprocal square root, one Jp dp term missing from a back-substitution or one
    landmark's E M^-1 g_l missing from the reduced gradient;
  - the E_REF2 table (the second step, tests/test_gpu_second_step.py) brackets the oracle's measured error against the twin's 50-digit
    LM loop, and the oracle accepts both steps;
  - expected_route restates BigPlan::choose at its edges."""
import numpy as np
import pytest

import step_helpers as sh
from oracle import twin
from sadvio_amd import capi, synthetic

mp = pytest.importorskip("mpmath")

WINDOWS = sorted({c.window: c for c in sh.CASES}.values(), key=lambda c: sh.CASES.index(c))


@pytest.mark.parametrize("factor", [capi.FACTOR_PIXEL, capi.FACTOR_ANGULAR])
def test_reference_matches_the_twins_unreduced_50_digit_solve(factor):
    """The arrowhead elimination + envelope Cholesky of mp_first_step against the twin's dense Cholesky of the whole system, both
    from the twin's 50-digit Jacobian (the oracle's float64 H would limit the comparison to 1e-16)."""
    w = synthetic.make_window(n_kf=3, n_lmk=14, obs_per_lmk=4, seed=5, factor=factor)
    opts = capi.reference_options()
    ref = twin.first_iteration(w, opts, kind="mp")
    B, P = ref["backend"], ref["problem"]
    _, _, r, J = P.evaluate(B.zeros(P.n))
    H, g = twin.normal_matrix(B, J), J.T @ r
    lay = sh.layout(w)
    assert lay["N"] == P.n and np.array_equal(lay["kf_off"], P.kf_col) and np.array_equal(lay["lmk_col"], P.lmk_col)   # same ordering
    got = sh.mp_first_step(w, opts, system=(H, g), want_cost=False)
    xp, xl = P.split(ref["x_scalar"])

    def rel(a, b):
        return max(abs(u - v) for u, v in zip(a.ravel(), b.ravel())) / max(abs(v) for v in b.ravel())
    assert rel(got["mp"]["pose"], xp) < 1e-25 and rel(got["mp"]["lmk"], xl) < 1e-25
    assert np.array_equal(got["pose"], ref["pose"]) and np.array_equal(got["lmk"], ref["lmk"])
    assert abs(got["mp"]["model_cost_change"] / mp.mpf(ref["log"][1][7]) - 1) < 1e-15     # the twin's log is rounded to float64
    # and the candidate cost (the twin's evaluation at mp_first_step's candidate)
    assert np.isclose(sh.mp_candidate_cost(w, got["mp"]), ref["log"][1][0], rtol=1e-15)


def test_envelope_cholesky_equals_the_dense_one_on_a_banded_system():
    mp.mp.dps = 50
    rng = np.random.default_rng(3)
    n, bw = 40, 5
    A = np.zeros((n, n))
    for i in range(n):
        for j in range(max(0, i - bw), i + 1):
            A[i, j] = A[j, i] = rng.standard_normal()
    A += 20.0 * np.eye(n)
    A[30, 2] = A[2, 30] = 0.5          # one long row: the envelope follows it
    b = rng.standard_normal(n)
    rows = [[mp.mpf(float(v)) for v in A[i, :i + 1]] for i in range(n)]
    y = sh.mp_envelope_cholesky_solve(rows, [mp.mpf(float(v)) for v in b])
    res = max(abs(mp.fdot([mp.mpf(float(v)) for v in A[i]], y) - mp.mpf(float(b[i]))) for i in range(n))
    assert res < 1e-45


@pytest.mark.parametrize("case", WINDOWS, ids=[c.window for c in WINDOWS])
def test_e_ref_table_brackets_the_measured_values(oracle_lib, case):
    """E_REF[window] >= the oracle's float64 error against the 50-digit step, and not more than 4 x above it; the oracle's trace row
    of the step agrees with the 50-digit model cost change and cost to the bar it is held to in test_twin.py."""
    w = case_w = sh.case_window(case)
    assert sh.reduced_np(w) == case.np_
    f64 = sh.oracle_step(oracle_lib, case_w, sh.case_options(case))
    ref = sh.reference(case, oracle_lib)
    e = sh.step_error(f64, ref, w)
    print(f"E_REF {case.window!r}: ({e[0]:.2e}, {e[1]:.2e}),")
    rec = sh.E_REF[case.window]
    for part, m, t in zip(("pose", "landmark"), e, rec):
        assert m <= t <= 4.0 * m, (part, m, t)
    assert np.isclose(f64["log"][1][7], ref["model_cost_change"], rtol=1e-11)
    assert np.isclose(f64["log"][1][0], ref["cost"], rtol=1e-11)


def _defects(N):
    last_block = 16 * ((N - 1) >> 4)
    return [("rsq seed on the first pivot", ("rsq", 0)), ("rsq seed on the last real pivot", ("rsq", N - 1)),
            ("rsq seed on the first pivot of the last block", ("rsq", last_block)), ("dropped rank-4 product", "product"),
            ("no damping on the last real column", "damping")]


@pytest.mark.parametrize("case", sh.LDS_CASES, ids=[c.name for c in sh.LDS_CASES])
def test_planted_defects_land_above_the_bar(oracle_lib, case):
    """Every defect must push the POSE part of the host model's step above the pose bar of the GPU test (a condition: a case that
    lets one through means the metric is too loose); the model without a defect stays within both bars."""
    w = sh.case_window(case)
    opts = capi.gn_options(1)
    H, g = sh.oracle_system(oracle_lib, w, opts)
    ref = sh.reference(case, oracle_lib)
    bar_p, bar_l = sh.bars(case)
    clean = sh.step_error(sh.host_model_step(w, H, g, opts), ref, w)
    assert clean[0] <= bar_p and clean[1] <= bar_l, ("the host model itself", clean, (bar_p, bar_l))
    missed = []
    for name, d in _defects(case.np_):
        e = sh.step_error(sh.host_model_step(w, H, g, opts, defect=d), ref, w)
        print(f"{case.name}: {name}: pose {e[0] / bar_p:.3g} x bar, landmark {e[1] / bar_l:.3g} x bar")
        if not e[0] > bar_p:
            missed.append((name, e, (bar_p, bar_l)))
    assert not missed, missed


@pytest.mark.parametrize("window", sh.SECOND_WINDOWS)
def test_e_ref2_table_brackets_the_measured_values(oracle_lib, window):
    """E_REF2[window] >= the C oracle's float64 error on the second step and on trace row 2 against the twin's 50-digit LM loop, and
    not more than 4 x above it; the oracle accepts both steps."""
    case = sh.window_case(window)
    w = sh.case_window(case)
    r1 = oracle_lib.solve(w, sh.case_options(case, 1))
    r2 = oracle_lib.solve(w, sh.case_options(case, 2))
    assert (r1["summary"].num_successful_steps, r2["summary"].num_successful_steps) == (1, 2), "the oracle rejects a step"
    ref = sh.second_reference(window)
    assert ref["pose"].shape == (w.n_kf, 6) and ref["lmk"].shape == (w.n_lmk, 3) and ref["row"][5] == 1.0
    e = sh.step_error(sh.second_step(r1, r2), ref, w) + (sh.row_error(r2["log"][2], ref["row"]),)
    print(f"E_REF2 {window!r}: ({e[0]:.2e}, {e[1]:.2e}, {e[2]:.2e}),")
    for part, m, t in zip(("pose", "landmark", "trace row 2"), e, sh.E_REF2[window]):
        assert m <= t <= 4.0 * m, (part, m, t)
    # the second step is a step of its own size, not the rounding of the first: the metric divides by max |second step|
    assert np.abs(sh.pose_part(ref, w)).max() > 1e-6 and np.abs(ref["lmk"]).max() > 1e-6


TILE_WINDOWS = [c for c in WINDOWS if c in sh.TILE_CASES and not c.route.endswith("extras")]
DEFECT_WINDOWS = ("w70", "lm_obs8", "g16", "w70_huber")


@pytest.mark.parametrize("case", TILE_WINDOWS, ids=[c.window for c in TILE_WINDOWS])
def test_tile_host_model_and_its_planted_defects(oracle_lib, case):
    """The clean host model of the tile kernels stays within both bars of the GPU test on every new window; on DEFECT_WINDOWS each
    planted defect pushes the pose or the landmark part above its bar (a condition: a window that lets one through is replaced,
    the bar is not moved)."""
    w = sh.case_window(case)
    opts = sh.case_options(case)
    ref = sh.reference(case, oracle_lib)
    bar_p, bar_l = sh.bars(case)
    clean = sh.step_error(sh.tile_host_model_step(w, opts), ref, w)
    print(f"{case.window}: clean host model: pose {clean[0] / bar_p:.3g} x bar, landmark {clean[1] / bar_l:.3g} x bar")
    assert clean[0] <= bar_p and clean[1] <= bar_l, ("the host model itself", clean, (bar_p, bar_l))
    if case.window not in DEFECT_WINDOWS:
        return
    missed = []
    for name in sh.TILE_DEFECTS:
        e = sh.step_error(sh.tile_host_model_step(w, opts, defect=name), ref, w)
        print(f"{case.window}: {name}: pose {e[0] / bar_p:.3g} x bar, landmark {e[1] / bar_l:.3g} x bar")
        if not (e[0] > bar_p or e[1] > bar_l):
            missed.append((name, e, (bar_p, bar_l)))
    assert not missed, missed


def test_expected_route_at_the_edges_of_the_plan():
    r = sh.expected_route
    assert r(174, 6, 174) == "lds" and r(165, 15, 45) == "lds"
    assert r(180, 6, 180) == "panel" and r(186, 6, 186) == "panel" and r(192, 6, 192) == "wide"       # dense: 2 x 96 columns
    assert r(180, 6, 18) == "band" and r(342, 6, 18) == "band" and r(180, 15, 45) == "band"
    assert r(378, 6, 18) == "band" and r(384, 6, 18) == "bcr"                                            # 21 / 22 blocks
    assert r(384, 6, 18, n_win=2) == "band" and r(384, 6, 18, no_bcr=True) == "band"
    assert r(641, 6, 18, no_bcr=True) == "band" and r(642, 6, 18, no_bcr=True) == "band_twisted"        # N - bw >= 4 x 156
    assert r(180, 6, 18, band_c=12) == "band_twisted" and r(65, 6, 18, band_c=12) == "lds"
    assert r(400, 6, 174) == "wide" and r(400, 6, 168) == "band_twisted"                                        # bw + 6 <= 174
    assert r(2000, 15, 45) == "band_twisted"                                                             # 5-column pivots: never bcr
    for c in sh.CASES:
        w = sh.case_window(c)
        lay = sh.layout(w)
        got = r(lay["Nr"], lay["dpf"], sh.band_rows(w), 1, int(c.env.get("SADVIO_BAND_C", 0)), c.env.get("SADVIO_NO_BCR") == "1")
        assert got == ("lds" if c.route.startswith("lds") else c.route), (c.name, got)
        assert sh.free_kf_observations(w).min() >= 10, c.name
