"""Long tracks on the device (sadvio_amd/csrc/long_kernels.h): landmarks of more than 64 observations are linearised, eliminated and
back-substituted by k_long_lin / k_long_back beside the tiles. Windows, references and bars: tests/long_track_helpers.py.

  1. first step    one LM step of every window against the 50-digit step, at TOL_FACTOR x max(E_REF, FLOOR) of step_helpers (pose,
                   landmark and IMU-state parts), model cost change and cost after the step to 1e-11 (the bar of test_gpu_first_step.py)
  2. both paths    MIX with SADVIO_LONG_MIN = 6, = 5 (its 5-observation landmarks on the long path too) and default, each in a
                   fresh child process, at the same 50-digit bar
  3. full solve    L65, MIX, BIG under the reference's options and GN-10 against oracle.solve, the bars of test_gpu_parity.py
  4. graph         use_graph = 1: a window without long tracks, one with, the first again, on ONE handle
  5. probes        linearize, landmark_chi2, landmark_chi2_models on L129
  6. refusals      the calls that do not serve long tracks say so and leave the solved state alone; caps; the sharded refusal

Every handle here is created with SADVIO_CFG_LONG_TRACKS (capi.Backend(long_tracks=True)); a handle without it refuses a 65th
observation as before (the last test). Every case prints its figures (`LONG ...`, run with -s) before it asserts."""
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import long_track_helpers as lh
import step_helpers as sh
from golden_util import assert_trace_matches, lmk_err
from sadvio_amd import capi, synthetic
from test_gpu_parity import LMK_TOL, POSE_TOL

pytestmark = pytest.mark.gpu
TESTS = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(autouse=True)
def _no_switch(monkeypatch):
    for k in sh.SWITCHES + ("SADVIO_LONG_MIN",):
        monkeypatch.delenv(k, raising=False)


def first_step(backend_cls, ws, i, opts, profile=True):
    be = backend_cls(device=0, profile_kernels=profile, long_tracks=True)
    try:
        be.set_windows(ws)
        sums = be.solve(opts)
        return sums, [be.get_deltas(k) for k in range(len(ws))], [be.get_trace(k) for k in range(len(ws))], be.kernel_times() if profile else {}
    finally:
        be.close()


def check_step(case, ref, s, d, tr, tag=""):
    w = lh.case_window(case)
    e = sh.step_error(d, ref, w)
    unit = [max(v, sh.FLOOR) for v in lh.E_REF[case.window]]
    mcc_rel = abs(tr[1][7] / ref["model_cost_change"] - 1) if len(tr) > 1 else np.inf
    cost_rel = abs(tr[1][0] / ref["cost"] - 1) if len(tr) > 1 else np.inf
    print(f"LONG first step {case.name}{tag}: Np {sh.reduced_np(w)} e_ref {lh.E_REF[case.window][0]:.1e} {lh.E_REF[case.window][1]:.1e} multiple pose {e[0] / unit[0]:.2f} "
          f"lmk {e[1] / unit[1]:.2f} (bar {sh.TOL_FACTOR:.0f}) mcc {mcc_rel:.1e} cost {cost_rel:.1e} steps {s.num_successful_steps}")
    assert s.num_successful_steps == 1
    bar_p, bar_l = lh.bars(case)
    assert e[0] <= bar_p, ("pose part", e[0], bar_p)
    assert e[1] <= bar_l, ("landmark part", e[1], bar_l)
    assert np.isclose(tr[1][7], ref["model_cost_change"], rtol=1e-11, atol=0)
    assert np.isclose(tr[1][0], ref["cost"], rtol=1e-11, atol=0)
    assert np.abs(d["pose"][np.asarray(w.kf_const) == 1]).max() == 0
    if getattr(w, "lmk_const", None) is not None:
        assert np.abs(d["lmk"][np.asarray(w.lmk_const) == 1]).max() == 0


# ---- 1. the first step -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", lh.CASES, ids=[c.name for c in lh.CASES])
def test_first_step_against_50_digits(backend_cls, oracle_lib, case):
    w = lh.case_window(case)
    sums, ds, trs, kt = first_step(backend_cls, [w], 0, lh.case_options(case))
    n = {k: v["launches"] for k, v in kt.items()}
    assert n.get("k_long_lin") == 1 and n.get("k_long_back") == 1 and n.get("k_build") == 1 and "k_lm_pass" not in n, n
    if case.name == "BIG":
        lay = sh.layout(w)
        assert lay["Nr"] == 240 > sh.MAX_LDS_NP and sh.band_rows(w) == lay["Nr"]          # out of LDS, and the long track fills the band
        assert "k_solve_front" in n and "k_solve" not in n, n
    check_step(case, lh.reference(case, oracle_lib), sums[0], ds[0], trs[0])


def test_first_step_in_a_batch_where_only_window_1_has_long_tracks(backend_cls, oracle_lib):
    c0, c1 = sh.CASE["w70"], lh.CASE["MIX"]
    w0, w1 = sh.case_window(c0), lh.case_window(c1)
    sums, ds, trs, kt = first_step(backend_cls, [w0, w1], 1, capi.gn_options(1))
    assert kt["k_long_lin"]["launches"] == 1 and kt["k_long_back"]["launches"] == 1
    check_step(c1, lh.reference(c1, oracle_lib), sums[1], ds[1], trs[1], tag="@1")
    ref0 = sh.reference(c0, oracle_lib)
    e = sh.step_error(ds[0], ref0, w0)
    bar_p, bar_l = sh.bars(c0)
    print(f"LONG first step w70@0 beside MIX: pose {e[0] / bar_p * sh.TOL_FACTOR:.2f} lmk {e[1] / bar_l * sh.TOL_FACTOR:.2f} of the unit (bar {sh.TOL_FACTOR:.0f})")
    assert e[0] <= bar_p and e[1] <= bar_l
    assert np.isclose(trs[0][1][7], ref0["model_cost_change"], rtol=1e-11, atol=0) and np.isclose(trs[0][1][0], ref0["cost"], rtol=1e-11, atol=0)


# ---- 2. the same window down both paths --------------------------------------------------------------------------------------------------
_CHILD = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.dirname(sys.argv[1]))
import numpy as np
import long_track_helpers as lh
from sadvio_amd import capi
case = lh.CASE[sys.argv[2]]
be = capi.Backend(device=0, profile_kernels=True, long_tracks=True)
be.set_windows([lh.case_window(case)])
s = be.solve(lh.case_options(case))[0]
d = be.get_deltas(0); tr = be.get_trace(0); kt = be.kernel_times()
be.close()
np.savez(sys.argv[3], trace=tr, steps=s.num_successful_steps, **d)
print(json.dumps({k: v["launches"] for k, v in kt.items()}))
"""


@pytest.mark.parametrize("long_min", ["6", "5", None])
def test_mix_down_both_paths(oracle_lib, tmp_path, long_min):
    case = lh.CASE["MIX"]
    env = dict(os.environ)
    env.pop("SADVIO_LONG_MIN", None)
    if long_min is not None:
        env["SADVIO_LONG_MIN"] = long_min
    out = str(tmp_path / "step.npz")
    p = subprocess.run([sys.executable, "-c", _CHILD, TESTS, case.name, out], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    n = json.loads(p.stdout.strip().splitlines()[-1])
    assert n.get("k_long_lin") == 1 and n.get("k_long_back") == 1, n
    z = np.load(out)
    s = dataclasses.make_dataclass("S", ["num_successful_steps"])(int(z["steps"]))
    check_step(case, lh.reference(case, oracle_lib), s, {k: z[k] for k in ("pose", "lmk", "dv", "dba", "dbg")}, z["trace"], tag=f" SADVIO_LONG_MIN={long_min}")


# ---- 3. the full solve -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["ref", "gn10"])
@pytest.mark.parametrize("name", ["L65", "MIX", "BIG"])
def test_full_solve_matches_oracle(backend_cls, oracle_lib, name, mode):
    w = lh.case_window(lh.CASE[name])
    opts = capi.reference_options() if mode == "ref" else capi.gn_options(10)
    be = backend_cls(device=0, long_tracks=True)
    try:
        be.set_windows([w])
        s = be.solve(opts)[0]
        d = be.get_deltas(0); tr = be.get_trace(0); ids = be.get_ids(0)
    finally:
        be.close()
    ref = oracle_lib.solve(w, opts)
    rs = ref["summary"]
    ep, el = np.abs(d["pose"] - ref["pose"]).max(), lmk_err(d["lmk"], ref["lmk"])
    print(f"LONG full solve {name} {mode}: iterations {s.iterations} / {rs.iterations} termination {s.termination} / {rs.termination} unsuccessful "
          f"{s.num_unsuccessful_steps} / {rs.num_unsuccessful_steps} pose {ep:.2e} lmk {el:.2e} (bar {POSE_TOL:.0e}) final cost {s.final_cost:.9g} / {rs.final_cost:.9g}")
    if (name, mode) in (("BIG", "ref"), ("L65", "gn10")):
        assert rs.num_unsuccessful_steps > 0                          # these solves contain rejected steps
    assert (s.iterations, s.termination) == (rs.iterations, rs.termination)
    assert np.isclose(s.final_cost, rs.final_cost, rtol=1e-9)
    assert ep <= POSE_TOL and el <= LMK_TOL
    n_rows = len(ref["log"]) - (1 if rs.termination in (1, 2) else 0)       # (the attempt that ends a solve through a tolerance is not applied)
    assert tr.shape == ref["log"].shape and np.allclose(tr[:n_rows, 0], ref["log"][:n_rows, 0], rtol=1e-9, atol=0)      # the cost after every iteration
    if mode == "ref":
        # (GN-10 has every early exit disabled: the attempts made after convergence accept / reject on cost changes of ~1e-12, rounding
        # noise, so step counts, radius and step quality are compared under the reference's options only, as test_gpu_parity.py does)
        assert (s.num_successful_steps, s.num_unsuccessful_steps) == (rs.num_successful_steps, rs.num_unsuccessful_steps)
        assert_trace_matches(tr, ref["log"], rs.termination)
    assert np.array_equal(ids[0], w.kf_id) and np.array_equal(ids[1], w.lmk_id)


# ---- 4. graph and re-plan ------------------------------------------------------------------------------------------------------------------
def _solve_fresh(backend_cls, w, opts, use_graph):
    be = backend_cls(device=0, use_graph=use_graph, long_tracks=True)
    try:
        be.set_windows([w])
        s = be.solve(opts)[0]
        return s, be.get_deltas(0)
    finally:
        be.close()


def test_graph_is_recaptured_when_long_tracks_come_and_go(backend_cls):
    """One handle with use_graph = 1: a window without long tracks, MIX, the first window again. The small window has 8 landmarks, so
    that one wave of one tile sums it and no sum depends on the order in which atomics arrive: its two solves on the handle and the
    solve of a fresh handle return the same bits. MIX's sums go through global atomics from several workgroups: there the solve on
    the re-planned handle equals a fresh handle's to 1e-10 relative (the figure of test_gpu_tile_packing.py's route comparison)."""
    small = synthetic.make_window(n_kf=4, n_lmk=8, obs_per_lmk=5, seed=9600)
    mix = lh.case_window(lh.CASE["MIX"])
    opts = capi.gn_options(4)
    be = backend_cls(device=0, use_graph=True, long_tracks=True)
    try:
        got = []
        for w in (small, mix, small):
            be.set_windows([w])
            s = be.solve(opts)[0]
            s2 = be.solve(opts)[0]                                  # the replay of the captured graph
            assert (s.iterations, s.final_cost) == (s2.iterations, s2.final_cost) or w is mix
            got.append((s2, be.get_deltas(0)))
    finally:
        be.close()
    fresh = [_solve_fresh(backend_cls, w, opts, True) for w in (small, mix)]
    for k in ("pose", "lmk"):
        assert got[0][1][k].tobytes() == got[2][1][k].tobytes() == fresh[0][1][k].tobytes(), k
    assert got[0][0].final_cost == got[2][0].final_cost == fresh[0][0].final_cost
    rel = lambda a, b: np.abs(a - b).max() / np.abs(b).max()
    fm = fresh[1]
    print(f"LONG graph: MIX on the re-planned handle against a fresh one: pose {rel(got[1][1]['pose'], fm[1]['pose']):.1e} lmk {rel(got[1][1]['lmk'], fm[1]['lmk']):.1e}")
    assert got[1][0].iterations == fm[0].iterations and abs(got[1][0].final_cost - fm[0].final_cost) <= 1e-10 * fm[0].final_cost
    assert rel(got[1][1]["pose"], fm[1]["pose"]) <= 1e-10 and rel(got[1][1]["lmk"], fm[1]["lmk"]) <= 1e-10


# ---- 5. the probes -----------------------------------------------------------------------------------------------------------------------
def test_probes_on_l129(backend_cls, oracle_lib):
    import camera_models as cm
    import model_gate_helpers as mg
    from test_gpu_window_index import CHI2_THRESHOLD_BAND, CHI2_TOL
    w = lh.case_window(lh.CASE["L129"])
    rng = np.random.default_rng(1)
    pd, ld = 0.01 * rng.standard_normal((w.n_kf, 6)), 0.03 * rng.standard_normal((w.n_lmk, 3))
    models = mg.pinhole_models(w)
    relerr = lambda a, b: np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)
    be = backend_cls(device=0, long_tracks=True)
    try:
        be.set_windows([w])
        for p, l in ((None, None), (pd, ld)):
            r, Jp, Jl = be.linearize(0, p, l)
            ro, Jpo, Jlo, _ = oracle_lib.linearize(w, p, l)
            print(f"LONG linearize L129: r {relerr(r, ro):.1e} Jp {relerr(Jp, Jpo):.1e} Jl {relerr(Jl, Jlo):.1e} (bar 1e-10)")
            assert relerr(r, ro) <= 1e-10 and relerr(Jp, Jpo) <= 1e-10 and relerr(Jl, Jlo) <= 1e-10
            kw = {} if p is None else {"pose_delta": p, "lmk_delta": l}
            avg, inl = be.landmark_chi2(0, **kw)
            ar, ir = oracle_lib.landmark_chi2(w, **kw)
            assert np.allclose(avg, ar, rtol=CHI2_TOL, atol=CHI2_TOL)
            sure = np.abs(ar - 2.0) > CHI2_THRESHOLD_BAND
            assert (inl[sure] == ir[sure]).all()
            mavg, minl, mobs = be.landmark_chi2_models(0, models, p, l, None, 1.0, want_obs=True)
            ravg, rinl, rterm = cm.chi2_gate(w, models, p, l, None, 1.0)
            ravg, rterm = cm.as_array(ravg), cm.as_array(rterm)
            print(f"LONG gates L129: chi2 {np.abs(avg - ar).max():.1e} models {np.abs(mavg - ravg).max():.1e} (bar {CHI2_TOL:.0e})")
            assert np.allclose(mavg, ravg, rtol=CHI2_TOL, atol=CHI2_TOL)
            sure = np.abs(ravg - 2.0) > CHI2_THRESHOLD_BAND
            assert (minl[sure] == rinl[sure]).all()
            for q in range(w.n_lmk):                                  # per observation: the landmark's terms, whatever order the slots are in
                o = slice(w.lmk_obs_ptr[q], w.lmk_obs_ptr[q + 1])
                assert np.allclose(np.sort(mobs[o]), np.sort(rterm[o]), rtol=CHI2_TOL, atol=CHI2_TOL)
    finally:
        be.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------
def _p2l(w, l, kf=0):
    from sparse_helpers import spd_sqrt
    T = np.asarray(w.kf_T_f_w[kf])
    return {"type": capi.SPARSE_POSE_TO_LMK, "kf": kf, "lmk0": l, "delta": T[:9].reshape(3, 3) @ w.lmk_p[l] + T[9:], "sqrt_inf": spd_sqrt(np.random.default_rng(3), 3, 8.0)}


def _set_sparse(be, w, factors):
    ws = dataclasses.replace(w, sparse_priors=factors, _keep=[])
    arr, n = ws.sparse_c()
    rc = be.lib.sadvio_ba_set_sparse_priors(be.h, 0, n, arr)
    return rc, be.lib.sadvio_ba_last_error(be.h).decode()


def test_calls_that_do_not_serve_long_tracks_refuse_and_leave_the_state_alone(backend_cls):
    w = lh.case_window(lh.CASE["MIX"])
    long_, short = int(lh.long_landmarks(w)[0]), 5
    assert lh.counts(w)[short] == 5
    prior = {"J": np.eye(3), "r0": np.zeros(3), "kf_keep": -1, "kf_col": 0, "lmk_index": [long_], "lmk_col": [0]}
    be = backend_cls(device=0, long_tracks=True)
    try:
        be.set_windows([w])
        be.solve(capi.gn_options(2))
        before = be.get_deltas(0)
        calls = {
            "covariance": lambda: be.covariance(0, kf=[0]),
            "covariance_batch": lambda: be.covariance_batch([{"w": 0, "kf": [0]}]),
            "covariance_cross": lambda: be.covariance_cross(0, kf=[0], lmk=[short]),
            "marginalize": lambda: be.marginalize(0, w.n_kf - 1, [], [short]),
            "marginalize_relative": lambda: be.marginalize_relative(0, 0, 1),
            "marginalize_relative_batch": lambda: be.marginalize_relative_batch(0, [(0, 1)]),
            "sparsify": lambda: be.sparsify(0, prior, vio=False),
            "set_dense_prior": lambda: be.set_dense_prior(0, prior),
        }
        for what, call in calls.items():
            with pytest.raises(capi.SadvioError) as ei:
                call()
            msg = str(ei.value)
            print(f"LONG refusal {what}: {msg}")
            assert f"rc={capi.E_INVALID_ARG}:" in msg and lh.LONG_TEXT in msg, (what, msg)
        rc, msg = _set_sparse(be, w, [_p2l(w, long_)])
        assert rc == capi.E_INVALID_ARG and lh.LONG_TEXT in msg, msg
        rc, msg = _set_sparse(be, w, [{"type": capi.SPARSE_LMK_PRIOR, "kf": -1, "lmk0": long_, "delta": w.lmk_p[long_], "sqrt_inf": np.eye(3)}])
        assert rc == capi.E_INVALID_ARG and lh.LONG_TEXT in msg, msg
        after = be.get_deltas(0)
        for k in before:
            assert before[k].tobytes() == after[k].tobytes(), k
        # priors on OTHER landmarks are served: a dense prior that keeps a short track, a pose-to-landmark factor on another
        be.set_dense_prior(0, dict(prior, lmk_index=[short]))
        s = be.solve(capi.gn_options(2))[0]
        assert s.iterations == 2 and np.isfinite(be.get_deltas(0)["lmk"]).all()
        be.set_dense_prior(0, None)
        rc, msg = _set_sparse(be, w, [_p2l(w, short + 1)])
        assert rc == capi.SADVIO_OK, msg
        s = be.solve(capi.gn_options(2))[0]
        assert s.iterations == 2 and np.isfinite(be.get_deltas(0)["lmk"]).all()
    finally:
        be.close()


def test_pseudo_observations_must_not_take_a_landmark_past_64(backend_cls):
    import test_gpu_tile_packing as tp
    full = lh.case_window(lh.CASE["L65"])
    w = tp._assemble(full, [(full, l, np.arange(63)) for l in range(full.n_lmk)])
    be = backend_cls(device=0, long_tracks=True)
    try:
        be.set_windows([w])
        rc, msg = _set_sparse(be, w, [_p2l(w, 0)])                    # 63 + 2 pseudo-observations
        assert rc == capi.E_INVALID_ARG and lh.LONG_TEXT in msg, msg
        with pytest.raises(capi.SadvioError) as ei:                   # and through the one-build bracket of set_windows
            be.set_windows([dataclasses.replace(w, sparse_priors=[_p2l(w, 0)], _keep=[])])
        assert lh.LONG_TEXT in str(ei.value)
    finally:
        be.close()


def test_a_sharded_handle_keeps_its_refusal_and_the_caps_have_their_own(backend_cls):
    import test_long_plan_cpu as tl
    w = lh.case_window(lh.CASE["L65"])
    be = backend_cls(device=0, long_tracks=True)
    try:
        be.set_collective(0, 2, lambda *a: 0)
        with pytest.raises(capi.SadvioError) as ei:
            be.set_windows([w])
        assert "a landmark has more than 64 observations" in str(ei.value) and lh.LONG_TEXT not in str(ei.value)
    finally:
        be.close()
    be = backend_cls(device=0)                                        # a handle that did not ask for long tracks (sadvio_ba_config.reserved = 0)
    try:
        with pytest.raises(capi.SadvioError) as ei:
            be.set_windows([w])
        assert "a landmark has more than 64 observations" in str(ei.value) and lh.LONG_TEXT not in str(ei.value)
    finally:
        be.close()
    be = backend_cls(device=0, long_tracks=True)
    try:
        for win, what, n in ((tl._shuffled_long_window(lh.MAX_LONG_OBS + 1), "observations", lh.MAX_LONG_OBS),
                             (tl._shuffled_long_window(2 * lh.MAX_LONG_KF + 2, n_kf=lh.MAX_LONG_KF + 1), "key-frames", lh.MAX_LONG_KF)):
            with pytest.raises(capi.SadvioError) as ei:
                be.set_windows([win])
            msg = str(ei.value)
            print(f"LONG cap: {msg}")
            assert f"rc={capi.E_INVALID_ARG}:" in msg and lh.LONG_TEXT in msg and what in msg and str(n) in msg
    finally:
        be.close()
