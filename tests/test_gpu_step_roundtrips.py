"""The places of the single-window step where memory round trips were taken off the chains (docs/KERNEL_HISTORY.md, "Round trips of
the step"), on windows that reach the branches the other suites do not:

  * k_solve's back half with more key-frames than SOLVE_KFC = 32 are parked in LDS: the parked loop (inputs and table through LDS,
    tables and step copied to HBM by the other waves) and the loop behind it (inputs from HBM) run in one launch. With 30 of 34
    key-frames fixed the tile image (N_p = 24: 768 doubles) is smaller than the 32 parked tables, which then leave the call as
    before; with 8 fixed (N_p = 156) they go through the image.
  * the Jacobi scales of a landmark, which k_build fetches with the first round's inputs and, in a later round of a multi-round
    tile, with that round's inputs: w70 as ONE three-round tile on the latency kernels, second step (slot 1 reads the scales slot 0
    wrote).
  * the per-iteration trace of the first window (its first tile's k_build writes the rows), with and without the graph, and on a
    solve that ends early so that the kernels of the remaining slots of a captured graph return through their `done` exits.

make_window(n_kf=34, n_lmk=400, fixed=30 | 8, band=2) at its default seed: the oracle accepts all three steps of gn_options(3),
every key-frame is observed (21 observations at least) and no landmark has more than 5 observations (checked below without a GPU)."""
import numpy as np
import pytest

import step_helpers as sh
from golden_util import assert_trace_matches, lmk_err
from sadvio_amd import capi, synthetic

POSE_TOL = 1e-6                   # test_gpu_parity.py's bars
LMK_TOL = 1e-6
FIXED = (30, 8)                   # 4 free key-frames (tables stored from the call), 26 (tables through the tile image)
EARLY_FTOL = 0.2                  # the third attempt changes the cost by 13 % (fixed = 30) / 9 % (fixed = 8): it ends the solve
_win, _ref = {}, {}


def window(fixed):
    if fixed not in _win:
        _win[fixed] = synthetic.make_window(n_kf=34, n_lmk=400, fixed=fixed, band=2)
    return _win[fixed]


def early_options():
    o = capi.reference_options()
    o.max_num_iterations = 8
    o.function_tolerance = EARLY_FTOL
    return o


def reference(oracle_lib, fixed, early=False):
    """The oracle's solve of the window, once per process."""
    if (fixed, early) not in _ref:
        _ref[fixed, early] = oracle_lib.solve(window(fixed), early_options() if early else capi.gn_options(3))
    return _ref[fixed, early]


@pytest.mark.parametrize("fixed", FIXED)
def test_windows_are_what_the_cases_say(oracle_lib, fixed):
    w = window(fixed)
    assert w.n_kf == 34 > 32 and int(np.sum(w.kf_const)) == fixed
    assert np.bincount(w.obs_kf, minlength=w.n_kf).min() > 0 and np.diff(w.lmk_obs_ptr).max() <= 64
    lay = sh.layout(w)
    assert lay["Nr"] == 6 * (34 - fixed) and sh.expected_route(lay["Nr"], 6, sh.band_rows(w)) == "lds"
    s = reference(oracle_lib, fixed)["summary"]
    assert (s.iterations, s.num_successful_steps) == (3, 3)
    s = reference(oracle_lib, fixed, early=True)["summary"]
    assert (s.num_successful_steps, s.termination) == (2, 1) and s.iterations < 8        # ended by the function tolerance


@pytest.mark.gpu
@pytest.mark.parametrize("fixed", FIXED)
def test_more_key_frames_than_parked(backend_cls, oracle_lib, fixed):
    w, opts = window(fixed), capi.gn_options(3)
    assert opts.jacobi_scaling == 1
    ref = reference(oracle_lib, fixed)
    be = backend_cls(device=0, profile_kernels=True)
    try:
        be.set_windows([w])
        s = be.solve(opts)[0]
        d = be.get_deltas(0)
        n = {k: v["launches"] for k, v in be.kernel_times().items()}
    finally:
        be.close()
    dp, dl = np.abs(d["pose"] - ref["pose"]).max(), lmk_err(d["lmk"], ref["lmk"])
    print(f"STEP_ROUNDTRIPS fixed {fixed} pose {dp:.2e} lmk {dl:.2e} cost {s.final_cost / ref['summary'].final_cost - 1:.1e} launches {n}")
    assert n.get("k_solve") == 3 and "k_solve_front" not in n, n          # the in-LDS solve
    assert dp <= POSE_TOL and dl <= LMK_TOL
    assert np.isclose(s.final_cost, ref["summary"].final_cost, rtol=1e-9, atol=0)
    assert s.num_successful_steps == ref["summary"].num_successful_steps == 3


@pytest.mark.gpu
def test_later_round_of_a_tile_at_a_later_slot(backend_cls, monkeypatch):
    """test_gpu_second_step.py's check of w70, on the latency kernels with the window as one three-round tile (SECOND_CASES has the
    three-round tile on the throughput kernels only)."""
    for k in sh.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SADVIO_TILE_ROUNDS", "3")
    case = sh.window_case("w70")
    w = sh.case_window(case)

    def solve(iters):
        be = backend_cls(device=0, profile_kernels=True)
        try:
            be.set_windows([w])
            s = be.solve(sh.case_options(case, iters))[0]
            return s, be.get_deltas(0), be.get_trace(0), {k: v["launches"] for k, v in be.kernel_times().items()}
        finally:
            be.close()

    s1, d1, _, _ = solve(1)
    s2, d2, tr, n = solve(2)
    ref = sh.second_reference("w70")
    e = sh.step_error(sh.second_step(d1, d2), ref, w)
    e_row = sh.row_error(tr[2], ref["row"]) if len(tr) > 2 else np.inf
    bar_p, bar_l, bar_row = sh.bars2("w70")
    print(f"STEP_ROUNDTRIPS w70 rounds3 latency pose {e[0]:.2e} (bar {bar_p:.1e}) lmk {e[1]:.2e} (bar {bar_l:.1e}) row {e_row:.1e} (bar {bar_row:.1e})")
    assert n.get("k_build") == 2 and n.get("k_backsub") == 2 and "k_lm_pass" not in n, n
    assert (s1.num_successful_steps, s2.num_successful_steps) == (1, 2)
    assert e[0] <= bar_p, ("pose part", e[0], bar_p)
    assert e[1] <= bar_l, ("landmark part", e[1], bar_l)
    assert e_row <= bar_row, ("trace row 2", e_row, bar_row)


@pytest.mark.gpu
@pytest.mark.parametrize("early", [False, True], ids=["three_steps", "ends_after_two"])
@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "stream"])
def test_trace_rows(backend_cls, oracle_lib, use_graph, early):
    w = window(FIXED[0])
    ref = reference(oracle_lib, FIXED[0], early)
    rs = ref["summary"]
    be = backend_cls(device=0, use_graph=use_graph)
    try:
        be.set_windows([w])
        s = be.solve(early_options() if early else capi.gn_options(3))[0]
        tr = be.get_trace(0)
    finally:
        be.close()
    assert (s.iterations, s.termination, s.num_successful_steps) == (rs.iterations, rs.termination, rs.num_successful_steps)
    assert_trace_matches(tr, ref["log"], rs.termination)
