"""sadvio_ba_landmark_chi2_models: the chi2 gate of ALandmark::sanityCheck with every observation projected by its camera's own
model, against the NumPy gate of tests/camera_models.py (which tests/test_camera_models_cpu.py holds to include/sadvio_cameras.hpp
and, at 50 digits, proves well conditioned on exactly these windows).

Bars: rtol = atol = 1e-9 on avg_chi2 and obs_chi2; inlier flags equal except where the reference's avg lies within 1e-6 of 2 (the
CHI2_TOL and CHI2_THRESHOLD_BAND of tests/test_gpu_window_index.py), and at most 2 % of the landmarks may lie in that band.
Windows: tests/model_gate_helpers.py (3 key-frames, 2 cameras of different kinds, 65 landmarks, tracks of 1, 2 and 5 observations,
every validity branch of every model). Every test prints its worst figure before it asserts."""
import dataclasses

import numpy as np
import pytest

import batch_helpers as bh
import camera_models as cm
import model_gate_helpers as mg
from sadvio_amd import capi
from sparse_helpers import spd_sqrt
from test_gpu_window_index import CHI2_THRESHOLD_BAND, CHI2_TOL

pytestmark = pytest.mark.gpu
PIXEL, ANGULAR = bh.PIXEL, bh.ANGULAR
FACTORS = [PIXEL, ANGULAR]
BAND_SHARE = 0.02


def reference(w, models, pd, ld, uv, sigma):
    avg, inl, term = cm.chi2_gate(w, models, pd, ld, uv, sigma)
    return cm.as_array(avg), inl, cm.as_array(term)


def compare(got, ref, what):
    """(worst avg figure, worst obs figure); asserts the bars."""
    (avg, inl, obs), (ravg, rinl, robs) = got, ref
    fa = (np.abs(avg - ravg) / (1.0 + np.abs(ravg))).max()
    fo = (np.abs(obs - robs) / (1.0 + np.abs(robs))).max()
    sure = np.abs(ravg - 2.0) > CHI2_THRESHOLD_BAND
    print(f"[model gate] {what}: worst |avg - ref| / (1 + |ref|) {fa:.3e}, per observation {fo:.3e}; bar rtol = atol = {CHI2_TOL:.0e}; "
          f"{(~sure).sum()} of {len(sure)} landmarks within {CHI2_THRESHOLD_BAND:.0e} of the threshold; inliers {inl.sum()}")
    assert np.allclose(avg, ravg, rtol=CHI2_TOL, atol=CHI2_TOL), what
    assert np.allclose(obs, robs, rtol=CHI2_TOL, atol=CHI2_TOL), what
    assert ((obs == 1000.0) == (robs == 1000.0)).all(), what
    assert (~sure).mean() <= BAND_SHARE, what
    assert (inl[sure] == rinl[sure]).all(), what
    return fa, fo


def run_states(be, k, w, models, uv, tag):
    """Window k of the handle at zero deltas, at fixed deltas and at the solved state, obs_uv given and NULL, both sigma choices."""
    d = be.get_deltas(k)
    states = [("zero", None, None), ("fixed",) + mg.fixed_deltas(w), ("solved", d["pose"], d["lmk"])]
    assert np.isfinite(d["pose"]).all() and np.isfinite(d["lmk"]).all()
    for name, pd, ld in states:
        for obs_uv in (uv, None):
            for sigma in ((1.0, 0.0) if name == "zero" else (1.0,)):
                got = be.landmark_chi2_models(k, models, pd, ld, obs_uv, sigma, want_obs=True)
                compare(got, reference(w, models, pd, ld, obs_uv, sigma), f"{tag}, {name} deltas, obs_uv {'given' if obs_uv is not None else 'NULL'}, sigma {sigma}")
    return be.landmark_chi2_models(k, models, None, None, uv, 1.0, want_obs=True)


@pytest.mark.parametrize("factor", FACTORS)
@pytest.mark.parametrize("rig", list(mg.RIGS))
def test_rig(backend_cls, rig, factor):
    w, models, uv = mg.rig_window(rig, factor)
    fisheye = [m["kind"] in cm.FISHEYE for m in models]
    be = backend_cls(device=0)
    try:
        be.set_windows([w])
        be.solve(capi.landmark_optimization_options())
        before = be.get_deltas(0)
        avg, inl, obs = run_states(be, 0, w, models, uv, f"{rig} factor {factor}")
        only_avg = be.landmark_chi2_models(0, models, obs_uv=uv, pixel_sigma=1.0)
        after = be.get_deltas(0)
    finally:
        be.close()
    assert np.array_equal(only_avg[0], avg) and np.array_equal(only_avg[1], inl)
    for key in before:                                   # the solved state stays readable
        assert np.array_equal(before[key], after[key]), key
    # the landmarks with a fixed role
    p = w.lmk_obs_ptr
    assert avg[mg.BEHIND] == 1000.0 and avg[mg.TOO_SHALLOW] == 1000.0 and avg[mg.OUTSIDE] == 1000.0
    shallow = obs[p[mg.SHALLOW]:p[mg.SHALLOW + 1]]
    for c, t in zip(w.obs_cam[p[mg.SHALLOW]:p[mg.SHALLOW + 1]], shallow):
        assert (t != 1000.0) == fisheye[c], "z = 0.05 passes the fisheye laws' depth test only"
    assert inl[mg.NEAR_AXIS] == 0 and avg[mg.NEAR_AXIS] < 10.0          # one observation: never an inlier, but projected
    assert 10 < inl.sum() < w.n_lmk - 5


@pytest.mark.parametrize("factor", FACTORS)
def test_pinhole_table_reproduces_landmark_chi2_bit_for_bit(backend_cls, factor):
    """sadvio_ba_landmark_chi2 and its kernel are unchanged; a table of pinholes must give its bits, at window 1 behind a decoy too."""
    t, a = bh.chi2_target(factor), bh.decoy(factor, "a")
    wh = np.tile([700.0, 460.0], (t.n_cam, 1))
    n = 0
    be = backend_cls(device=0)
    try:
        for ws, k in (([t], 0), ([a, t], 1)):
            be.set_windows(ws)
            be.solve(capi.landmark_optimization_options())
            d = be.get_deltas(k)
            for kw in ({}, {"lmk_delta": d["lmk"]}, {"lmk_delta": d["lmk"], "pose_delta": 0.003 * np.ones((t.n_kf, 6))}):
                for image_wh in (None, wh):
                    for sigma in (0.0, 1.0, 1.7):
                        avg, inl = be.landmark_chi2(k, image_wh=image_wh, pixel_sigma=sigma, **kw)
                        got = be.landmark_chi2_models(k, mg.pinhole_models(t, image_wh), pixel_sigma=sigma, want_obs=True, **kw)
                        assert avg.tobytes() == got[0].tobytes() and np.array_equal(inl, got[1]), (k, kw.keys(), image_wh is None, sigma)
                        per_lmk = np.add.reduceat(got[2], t.lmk_obs_ptr[:-1]) / np.diff(t.lmk_obs_ptr)
                        assert np.allclose(per_lmk, avg, rtol=1e-12, atol=0)
                        n += 1
            assert (avg == 1000.0).any() and 0 < inl.sum() < t.n_lmk
    finally:
        be.close()
    print(f"[model gate] factor {factor}: {n} calls, avg_chi2 of a pinhole table bit-identical to sadvio_ba_landmark_chi2")


@pytest.mark.parametrize("factor", FACTORS)
def test_window_index(backend_cls, factor):
    """The target is window 2 of 3; the decoys in front carry 3 and 1 cameras of other kinds (cam_base = 4), other key-frame,
    landmark and observation counts, and are evaluated themselves, before and between the calls on the target. A table row read
    without the window's camera base is a decoy's or no row at all (tests/test_camera_models_cpu.py: a decoy's row shows)."""
    (a, ma, uva), (b, mb, uvb), (t, mt, uvt) = mg.decoys(factor) + (mg.target(factor),)
    be = backend_cls(device=0)
    try:
        be.set_windows([a, b, t])
        be.solve(capi.landmark_optimization_options())
        before = [be.get_deltas(i) for i in range(3)]
        for k, (w, m, uv) in ((0, (a, ma, uva)), (1, (b, mb, uvb)), (2, (t, mt, uvt)), (0, (a, ma, uva)), (2, (t, mt, uvt))):
            run_states(be, k, w, m, uv, f"window {k} of [a, b, target] factor {factor}")
        after = [be.get_deltas(i) for i in range(3)]
    finally:
        be.close()
    for x, y in zip(before, after):
        for key in x:
            assert np.array_equal(x[key], y[key]), key


@pytest.mark.parametrize("factor", FACTORS)
def test_sparse_prior_pseudo_observation_is_skipped(backend_cls, factor):
    """One sparse pose-to-landmark prior factor rides the elimination as two pseudo-observations of its landmark (cam < 0 in the
    stored lists). The gate skips them: same bits as without the factor, and obs_chi2 keeps the caller's n_obs slots."""
    w, models, uv = mg.target(factor)
    l = 5                                                           # five observations, free
    assert w.lmk_obs_ptr[l + 1] - w.lmk_obs_ptr[l] == 5
    T = np.asarray(w.kf_T_f_w[0])
    delta = T[:9].reshape(3, 3) @ w.lmk_p[l] + T[9:] + 0.01
    ws = dataclasses.replace(w, sparse_priors=[{"type": capi.SPARSE_POSE_TO_LMK, "kf": 0, "lmk0": l, "delta": delta,
                                                "sqrt_inf": spd_sqrt(np.random.default_rng(3), 3, 8.0)}], _keep=[])
    be = backend_cls(device=0)
    try:
        be.set_windows([w])
        plain = [be.landmark_chi2_models(0, models, obs_uv=u, pixel_sigma=1.0, want_obs=True) for u in (uv, None)]
        be.set_windows([ws])
        withf = [be.landmark_chi2_models(0, models, obs_uv=u, pixel_sigma=1.0, want_obs=True) for u in (uv, None)]
        r = be.linearize(0)[0]
    finally:
        be.close()
    assert r.shape[0] == w.n_obs
    for p, q, u in zip(plain, withf, (uv, None)):
        assert q[2].shape == (w.n_obs,)
        for x, y in zip(p, q):
            assert x.tobytes() == y.tobytes()
        compare(q, reference(w, models, None, None, u, 1.0), f"sparse prior factor, factor {factor}, obs_uv {'given' if u is not None else 'NULL'}")


def test_error_codes_leave_outputs_and_state_untouched(backend_cls):
    w, models, uv = mg.target(ANGULAR)
    twin = dataclasses.replace(w, cam_K=np.vstack([w.cam_K[0], w.cam_K[0]]), cam_T_s_f=np.vstack([w.cam_T_s_f[0], w.cam_T_s_f[0]]),
                               cam_sigma=np.array([w.cam_sigma[0], w.cam_sigma[0]]), _keep=[])      # the handle stores ONE camera

    def untouched(out):
        return all(np.isnan(x).all() if x.dtype == np.float64 else (x == -1).all() for x in out)

    def call(be, k, m, **kw):
        rc, *out = be.landmark_chi2_models(k, m, obs_uv=uv, pixel_sigma=1.0, want_obs=True, raw_rc=True, **kw)
        return rc, out

    be = backend_cls(device=0)
    try:
        be.windows = [w]                                              # sizes the output arrays; nothing is uploaded
        rc, out = call(be, 0, models)
        assert rc == capi.E_STATE and untouched(out), "before set_windows"
        be.set_windows([w])
        be.solve(capi.landmark_optimization_options())
        before = be.get_deltas(0)
        ok = be.landmark_chi2_models(0, models, obs_uv=uv, pixel_sigma=1.0, want_obs=True)
        assert be.lib.sadvio_ba_begin_update(be.h) == capi.SADVIO_OK
        rc, out = call(be, 0, models)
        assert be.lib.sadvio_ba_commit_update(be.h) == capi.SADVIO_OK
        assert rc == capi.E_STATE and untouched(out), "inside a begin_update bracket"
        bad_kind = [dict(models[0]), dict(models[1], kind=6)]
        negative = [dict(models[0], kind=-1), dict(models[1])]
        for what, k, m in (("null models", 0, None), ("unknown kind", 0, bad_kind), ("negative kind", 0, negative)):
            rc, out = call(be, k, m)
            assert rc == capi.E_INVALID_ARG and untouched(out), what
        for k in (-1, 1):
            avg = np.full(w.n_lmk, np.nan)
            rc = be.lib.sadvio_ba_landmark_chi2_models(be.h, k, None, None, capi.camera_models_c(models), None, 1.0, capi._ptr(avg), None, None)
            assert rc == capi.E_INVALID_ARG and np.isnan(avg).all(), "window out of range"
        again = be.landmark_chi2_models(0, models, obs_uv=uv, pixel_sigma=1.0, want_obs=True)
        after = be.get_deltas(0)
        # two window cameras the handle stores once: their models and image sizes must agree
        be.set_windows([twin])
        same = [dict(models[1]), dict(models[1])]
        rc, out = call(be, 0, same)
        assert rc == capi.SADVIO_OK and not untouched(out)
        for what, m in (("kinds differ", [dict(models[1]), dict(models[0])]), ("image sizes differ", [dict(models[1]), dict(models[1], width=700.0)]),
                        ("rmax differs", [dict(models[1]), dict(models[1], rmax=299.0)])):
            rc, out = call(be, 0, m)
            assert rc == capi.E_INVALID_ARG and untouched(out), what
    finally:
        be.close()
    for x, y in zip(ok, again):
        assert x.tobytes() == y.tobytes()
    for key in before:
        assert before[key].tobytes() == after[key].tobytes(), key
