"""sadvio_ba_covariance_cross on the device against blocks of the float64 inverse of the FULL information matrix
(tests/cov_cross_helpers.py), evaluated at the deltas the device's own solve returned. A cross block passes when
max |got - ref| / sqrt(max |X_aa| max |X_ll|) is at most TOL_FACTOR = 64 x E_REF_CROSS of its window; P (cov_helpers.rel_diff) and
maha2 (|got - ref| / max(ref, 1)) at 64 x E_REF_INNOV — the figures float64 itself loses against a 50-digit inverse
(tests/test_cov_cross_cpu.py). The candidate observations are the window's own where it has one, else the predicted measurement plus
an offset; candidates whose landmark projects outside the image or behind the camera (there are some on every pixel window; the
tests assert it) must come back as SADVIO_CROSS_PROJ_INVALID with maha2 = 0. Every test prints its worst figure before it asserts.

The 345-key-frame window (N_p = 2 064, the band route by default) is held against the block-sparse Schur reference."""
import dataclasses

import numpy as np
import pytest

import batch_helpers as bt
import cov_band_helpers as bh
import cov_cross_helpers as xh
import cov_helpers as ch
from sadvio_amd import capi, synthetic

pytestmark = pytest.mark.gpu


def _opts(huber=0.0):
    o = capi.reference_options()
    o.huber_a = huber
    return o


def _env(monkeypatch, **kw):
    for key in ("SADVIO_COV_SQRT", "SADVIO_COV_BAND", "SADVIO_COV_CROSS_STAGE"):
        monkeypatch.delenv(key, raising=False)
    for key, val in kw.items():
        monkeypatch.setenv("SADVIO_COV_" + key.upper(), str(val))


def _run(backend_cls, w, huber, kf, lmk, innov=True, profile=False):
    """Solve, then one cross call: (deltas, cam, meas, result, kernel classes)."""
    be = backend_cls(device=0, profile_kernels=True) if profile else backend_cls(device=0)
    try:
        be.set_windows([w])
        be.solve(_opts(huber))
        d = be.get_deltas(0)
        cam, meas = xh.candidate_observations(w, d, kf, lmk) if innov else (None, None)
        got = be.covariance_cross(0, kf, lmk, cam, meas)
        kt = be.kernel_times() if profile else {}
    finally:
        be.close()
    return d, cam, meas, got, kt


def _check(case, w, d, kf, lmk, cam, meas, got, huber=0.0, w_ref=None, label=""):
    wr = w_ref if w_ref is not None else w
    info = ch.Information(wr, d, huber)
    X = np.linalg.inv(info.H)
    e_cross, e_innov = xh.worst_errors(wr, info, X, d, kf, lmk, cam, meas, got)
    t_cross = ch.TOL_FACTOR * xh.E_REF_CROSS[case]
    t_innov = ch.TOL_FACTOR * xh.E_REF_INNOV[case] if cam is not None else float("nan")
    print(f"[cov cross] {case}{label}: {len(kf)} candidates, worst cross {e_cross:.3e} (bound {t_cross:.3e}), innovation {e_innov:.3e} (bound {t_innov:.3e})")
    assert e_cross <= t_cross, (case, e_cross, t_cross)
    if cam is not None:
        assert e_innov <= t_innov, (case, e_innov, t_innov)
        inv = got["status"] == xh.CROSS_PROJ_INVALID
        assert np.all(got["maha2"][inv] == 0.0) and np.isfinite(got["innov"][inv]).all()
        ok = got["status"] == xh.CROSS_OK
        assert np.all(got["maha2"][ok] >= 0.0) and np.array_equal(got["innov"][ok][:, 0, 1], got["innov"][ok][:, 1, 0])
    return info, X


def _case(backend_cls, case, innov=True):
    build, huber, cands = xh.CASES[case]
    w = build()
    kf, lmk = cands(w)
    d, cam, meas, got, _ = _run(backend_cls, w, huber, kf, lmk, innov)
    info, X = _check(case, w, d, kf, lmk, cam, meas, got, huber)
    return w, kf, lmk, got, info


def test_pixel_vo_every_combination(backend_cls):
    """N_p = 12: every (key-frame, landmark) pair, 120 candidates — the constant key-frame (zeros), the single-observation landmark
    (NaN, SADVIO_CROSS_LMK_SINGULAR), own observations and unobserved pairs, projections outside the image."""
    w, kf, lmk, got, info = _case(backend_cls, "pixel_vo")
    assert len(kf) == 120 and info.singular == [ch.SINGLE]
    sing = lmk == ch.SINGLE
    assert np.isnan(got["cross"][sing]).all() and np.isnan(got["innov"][sing]).all() and np.isnan(got["maha2"][sing]).all()
    assert np.all(got["status"][sing] == xh.CROSS_LMK_SINGULAR)
    const = (kf == w.n_kf - 1) & ~sing
    assert np.all(got["cross"][const] == 0.0) and np.all(got["innov"][const][:, 0, 0] > 1.0)   # P = J_l Sigma_ll J_l^T + I
    assert (got["status"] == xh.CROSS_PROJ_INVALID).sum() >= 1 and (got["status"] == xh.CROSS_OK).sum() >= 60
    free = ~const & ~sing
    assert np.all(np.abs(got["cross"][free]).max(axis=(1, 2)) > 0.0)


def test_angular_vo(backend_cls):
    """N_p = 18, unit-bearing measurements."""
    w, kf, lmk, got, _ = _case(backend_cls, "angular_vo")
    assert np.all(got["status"] == xh.CROSS_OK)


def test_huber(backend_cls):
    """The window's own factors under the solve's Huber corrector; the candidate's residual without a loss."""
    _case(backend_cls, "huber")


def test_constant_landmark(backend_cls):
    """lmk_const landmarks: Sigma_al = 0 and P = J_a Sigma_aa J_a^T + I."""
    w = ch.window_angular_vo()
    w.lmk_const = np.zeros(w.n_lmk, dtype=np.uint8)
    w.lmk_const[[3, 17]] = 1
    kf, lmk = xh.CASES["angular_vo"][2](w)
    d, cam, meas, got, _ = _run(backend_cls, w, 0.0, kf, lmk)
    _check("angular_vo", w, d, kf, lmk, cam, meas, got)
    c = np.isin(lmk, [3, 17])
    assert np.all(got["cross"][c] == 0.0) and np.all(got["status"][c] == xh.CROSS_OK)


def test_vio_with_the_resident_dense_prior(backend_cls):
    """d = 15 (45 of 64 lanes per candidate); the prior-kept landmarks' cross blocks are read from Sigma_pp."""
    w, args, w2, keep = ch.vio_marg_step()
    be = backend_cls(device=0)
    try:
        be.set_prior(ch.VIO_J0, np.zeros(15))
        be.set_windows([w])
        g = be.marginalize(0, form="cholesky", readback=True, **args)
        assert g is not None and g["n_full"] == g["n"]
        w_ref = ch.vio_attach(w, w2, keep, g, None)
        w_dev = dataclasses.replace(w_ref, dense_prior=dict({k: v for k, v in w_ref.dense_prior.items() if k not in ("J", "r0")}, resident=True))
        be.set_windows([w_dev])
        be.solve(_opts())
        d = be.get_deltas(0)
        kf, lmk = xh.CASES["vio_dense"][2](w_ref)
        cam, meas = xh.candidate_observations(w_ref, d, kf, lmk)
        got = be.covariance_cross(0, kf, lmk, cam, meas)
    finally:
        be.close()
    assert got["cross"].shape == (len(kf), 15, 3)
    _check("vio_dense", w_dev, d, kf, lmk, cam, meas, got, w_ref=w_ref)
    kept = [int(np.flatnonzero(w_ref.lmk_id == w.lmk_id[l])[0]) for l in keep if len(np.flatnonzero(w_ref.lmk_id == w.lmk_id[l]))]
    assert len(kept) >= 1 and np.all(np.abs(got["cross"][np.isin(lmk, kept)]).max(axis=(1, 2)) > 0.0)


def test_landmark_with_64_observations(backend_cls):
    """Landmark OBS64_LMK x all 32 key-frames: the longest entry loop (31 entries)."""
    _case(backend_cls, "obs64")


def test_newest_key_frame_by_every_landmark_shuffled_with_repeats(backend_cls, monkeypatch):
    """605 landmarks x the newest key-frame in a shuffled order with repeats: several workgroups per key-frame, group boundaries,
    output order. Then the same request with the LDS staging limit exactly at the block row's size (6 x 42 = 252 doubles: staged) and
    one below it (read from global memory): within the bar, and the same bits where the run's solve returned the same deltas."""
    build, huber, cands = xh.CASES["lmk600"]
    w = build()
    kf0, lmk0 = cands(w)
    rng = np.random.default_rng(5)
    sel = np.concatenate([rng.permutation(len(kf0)), rng.integers(0, len(kf0), 90)])
    kf, lmk = kf0[sel], lmk0[sel]
    assert len(kf) > 7 * 96                                           # more than seven workgroups of one key-frame
    outs = []
    for stage in (None, 252, 251):
        _env(monkeypatch, **({} if stage is None else {"cross_stage": stage}))
        d, cam, meas, got, _ = _run(backend_cls, w, huber, kf, lmk)
        _check("lmk600", w, d, kf, lmk, cam, meas, got, huber, label=f" [stage {stage}]")
        outs.append((d, got))
    first = {}
    for i, s in enumerate(sel):                                       # a repeat returns the bits of its first occurrence
        j = first.setdefault(int(s), i)
        assert outs[0][1]["cross"][i].tobytes() == outs[0][1]["cross"][j].tobytes()
    for d, got in outs[1:]:   # (the limit is read when the handle is created: each run has its own solve, held to the bar above)
        same = all(d[k].tobytes() == outs[0][0][k].tobytes() for k in d)
        print(f"[cov cross] lmk600: deltas bit-identical to the first run: {same}")
        if same:
            assert got["cross"].tobytes() == outs[0][1]["cross"].tobytes()


def test_position_and_company_do_not_change_a_candidate(backend_cls):
    """A candidate alone, and among 159 others at another position: the same bits."""
    w = ch.window_angular_vo()
    kf, lmk = xh.CASES["angular_vo"][2](w)
    be = backend_cls(device=0)
    try:
        be.set_windows([w]); be.solve(_opts())
        d = be.get_deltas(0)
        cam, meas = xh.candidate_observations(w, d, kf, lmk)
        a = be.covariance_cross(0, kf, lmk, cam, meas)
        i = 77
        b = be.covariance_cross(0, kf[i:i + 1], lmk[i:i + 1], cam[i:i + 1], meas[i:i + 1])
        c = be.covariance_cross(0, kf[::-1], lmk[::-1], cam[::-1], meas[::-1])
    finally:
        be.close()
    for key in ("cross", "innov", "maha2", "status"):
        assert a[key][i].tobytes() == b[key][0].tobytes(), key
        assert a[key].tobytes() == c[key][::-1].tobytes(), key


# ---- the square-root assembly -------------------------------------------------------------------------------------------------------
def test_square_root_assembly_pixel_vo(backend_cls, monkeypatch):
    _env(monkeypatch, sqrt=1)
    build, huber, cands = xh.CASES["pixel_vo"]
    w = build()
    kf, lmk = cands(w)
    d, cam, meas, got, kt = _run(backend_cls, w, huber, kf, lmk, profile=True)
    assert "cov_assemble_sqrt" in kt and "cov_assemble" not in kt and "cov_cross" in kt
    _check("pixel_vo", w, d, kf, lmk, cam, meas, got, label=" [SADVIO_COV_SQRT=1]")


def test_square_root_assembly_near_camera_landmark(backend_cls, monkeypatch):
    """A landmark 1 mm from a camera centre under SADVIO_COV_SQRT=1: cross blocks of NEAR_LMK with every key-frame (no innovation
    yardstick on these windows, see cov_cross_helpers). At 0.1 mm, with the variable unset, the plain assembly is refused by the
    pivot tests and the call is served through the retry."""
    _env(monkeypatch, sqrt=1)
    _case(backend_cls, "near_1e-3", innov=False)
    _env(monkeypatch)
    build, huber, cands = xh.CASES["near_1e-4"]
    w = build()
    kf, lmk = cands(w)
    d, _, _, got, kt = _run(backend_cls, w, huber, kf, lmk, innov=False, profile=True)
    assert "cov_assemble" in kt and "cov_assemble_sqrt" in kt          # the plain attempt, then the retry
    _check("near_1e-4", w, d, kf, lmk, None, None, got, label=" [through the retry]")
    d, cam, meas, got, _ = _run(backend_cls, w, huber, kf, lmk, innov=True)
    ok = got["status"] == xh.CROSS_OK
    assert np.isfinite(got["innov"]).all() and np.all(got["maha2"][ok] >= 0.0) and np.all(got["innov"][:, 0, 0] >= 1.0)


# ---- the band route -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["vo12", "vio8"])
def test_band_route(backend_cls, monkeypatch, case):
    """SADVIO_COV_BAND=1: key-frames inside, below and above the band of the landmark's observers, the first and the last free
    key-frame and the constant one; every candidate is served from the solved block row. Two requests that share candidates return
    the same bits for them."""
    _env(monkeypatch, band=1)
    build, huber, cands = xh.CASES[case]
    w = build()
    kf, lmk = cands(w)
    hb, bw, dpf = bh.bandwidth(w)
    f = bh.free_index(w)
    lo = np.array([f[w.obs_kf[w.lmk_obs_ptr[l]:w.lmk_obs_ptr[l + 1]]].min() for l in lmk])
    hi = np.array([f[w.obs_kf[w.lmk_obs_ptr[l]:w.lmk_obs_ptr[l + 1]]].max() for l in lmk])
    fa = f[kf]
    assert ((fa >= 0) & (fa < lo - hb)).any() and ((fa > hi + hb)).any() and ((fa >= lo) & (fa <= hi)).any()
    assert (fa == 0).any() and (fa == f.max()).any() and (fa < 0).any()
    be = backend_cls(device=0, profile_kernels=True)
    try:
        be.set_windows([w]); be.solve(_opts(huber))
        d = be.get_deltas(0)
        cam, meas = xh.candidate_observations(w, d, kf, lmk)
        got = be.covariance_cross(0, kf, lmk, cam, meas)
        kt = be.kernel_times()
        sub = np.arange(5, len(kf), 3)
        part = be.covariance_cross(0, kf[sub], lmk[sub], cam[sub], meas[sub])
    finally:
        be.close()
    assert "cov_band_rows" in kt and "cov_band" in kt and "cov_cross" in kt and "cov_invert" not in kt
    _check(case, w, d, kf, lmk, cam, meas, got, huber, label=f" [band route, hb {hb}, bw {bw}]")
    for key in ("cross", "innov", "maha2", "status"):
        assert part[key].tobytes() == got[key][sub].tobytes(), key


def test_default_route_at_2064_columns(backend_cls, monkeypatch):
    """No variable set. 345 key-frames, N_p = 2 064: the band route by default, the 99 KB block row staged in LDS. The first, middle
    and last free key-frame x 20 landmarks against the block-sparse Schur reference at the device's own deltas."""
    _env(monkeypatch)
    w = bh.window_at_size()
    hb, bw, _ = bh.bandwidth(w)
    kf, lmk = xh.at_size_candidates(w)
    assert 6 * int((w.kf_const == 0).sum()) == 2064 and len(kf) == 60
    be = backend_cls(device=0, profile_kernels=True)
    try:
        be.set_windows([w]); be.solve(_opts())
        d = be.get_deltas(0)
        cam, meas = xh.candidate_observations(w, d, kf, lmk)
        got = be.covariance_cross(0, kf, lmk, cam, meas)
        kt = be.kernel_times()
    finally:
        be.close()
    assert "cov_band_rows" in kt and "cov_cross" in kt and "cov_invert" not in kt, sorted(kt)
    info, X = xh.at_size_reference(bh.SchurBlocks(w, d), bw, kf, lmk)
    e_cross, e_innov = xh.worst_errors(w, info, X, d, kf, lmk, cam, meas, got)
    t_cross, t_innov = ch.TOL_FACTOR * xh.E_REF_CROSS["at_size"], ch.TOL_FACTOR * xh.E_REF_INNOV["at_size"]
    print(f"[cov cross] at_size: N_p 2064, hb {hb}, bw {bw}, {len(kf)} candidates, worst cross {e_cross:.3e} (bound {t_cross:.3e}), "
          f"innovation {e_innov:.3e} (bound {t_innov:.3e})")
    assert e_cross <= t_cross and e_innov <= t_innov


# ---- contract ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(backend_cls, monkeypatch):
    from line_helpers import add_lines
    from sadvio_amd import sharding
    w = ch.window_angular_vo()
    b3 = np.array([[0.0, 0.0, 1.0]])
    be = backend_cls(device=0)
    try:
        be.set_windows([w])
        r = be.covariance_cross(0, [0], [0], raw_rc=True)
        assert r["rc"] == capi.E_STATE and "before solve" in r["error"]
        be.solve(_opts())
        for kw in (dict(kf=[4], lmk=[0]), dict(kf=[-1], lmk=[0]), dict(kf=[0], lmk=[w.n_lmk]), dict(kf=[0], lmk=[-2]),
                   dict(kf=[0], lmk=[0], cam=[2], meas=b3), dict(kf=[0], lmk=[0], cam=[-1], meas=b3)):
            r = be.covariance_cross(0, raw_rc=True, **kw)
            assert r["rc"] == capi.E_INVALID_ARG and "out of range" in r["error"], kw
        r = be.covariance_cross(0, [0], [0], raw_rc=True, want_innov=True)            # innov_cov / maha2 with cam == NULL
        assert r["rc"] == capi.E_INVALID_ARG and "innovation" in r["error"]
        assert be.covariance_cross(1, [0], [0], raw_rc=True)["rc"] == capi.E_INVALID_ARG
        r = be.covariance_cross(0, [], [])                                             # n = 0
        assert r["rc"] == 0 and r["cross"].shape == (0, 6, 3)
        be._check(be.lib.sadvio_ba_begin_update(be.h), "begin_update")
        r = be.covariance_cross(0, [0], [0], raw_rc=True)
        be._check(be.lib.sadvio_ba_commit_update(be.h), "commit_update")
        assert r["rc"] == capi.E_STATE and "begin_update" in r["error"]
    finally:
        be.close()
    wl = add_lines(synthetic.make_window(n_kf=4, n_lmk=60, obs_per_lmk=4, seed=21), n_line=3, obs_per_line=4)
    be = backend_cls(device=0)
    try:
        be.set_windows([wl]); be.solve(_opts())
        r = be.covariance_cross(0, [0], [0], raw_rc=True)
        assert r["rc"] == capi.E_INVALID_ARG and "line landmarks" in r["error"]
    finally:
        be.close()
    be = backend_cls(device=0)
    try:
        be.set_collective(0, 2, lambda *a: 0)
        be.set_windows([sharding.shard_window(synthetic.make_window(n_kf=5, n_lmk=300, seed=42), 0, 2)])
        r = be.covariance_cross(0, [0], [0], raw_rc=True)
        assert r["rc"] == capi.E_INVALID_ARG and "sharded" in r["error"]
    finally:
        be.close()
    monkeypatch.setenv("SADVIO_LM", "1")
    be = backend_cls(device=0)
    try:
        be.set_windows([synthetic.make_window(n_kf=6, n_lmk=400, seed=7)]); be.solve(_opts())
        r = be.covariance_cross(0, [0], [0], raw_rc=True)
        assert r["rc"] == capi.E_INVALID_ARG and "throughput" in r["error"]
    finally:
        be.close()


def test_unanchored_window_is_not_usable(backend_cls):
    w = synthetic.make_window(n_kf=4, n_lmk=60, obs_per_lmk=4, seed=33, fixed=0)
    w.pose_priors = []
    be = backend_cls(device=0)
    try:
        be.set_windows([w]); be.solve(_opts())
        d = be.get_deltas(0)
        kf, lmk = np.array([0, 1, 2], dtype=np.int32), np.array([3, 4, 5], dtype=np.int32)
        cam, meas = xh.candidate_observations(w, d, kf, lmk)
        r = be.covariance_cross(0, kf, lmk, cam, meas, raw_rc=True)
    finally:
        be.close()
    assert r["rc"] == capi.E_NOT_USABLE and "positive definite" in r["error"]
    assert np.all(r["cross"] == 0.0) and np.all(r["innov"] == 0.0) and np.all(r["maha2"] == 0.0) and np.all(r["status"] == 0)


def test_solve_results_and_covariance_untouched_and_two_calls_identical(backend_cls):
    w = ch.window_pixel_vo()
    kf, lmk = xh.CASES["pixel_vo"][2](w)
    be = backend_cls(device=0)
    try:
        be.set_windows([w]); be.solve(_opts())
        d0, t0 = be.get_deltas(0), be.get_trace(0)
        c0 = be.covariance(0, kf=[0, 1, 2], pairs=[(0, 1)], lmk="all")
        cam, meas = xh.candidate_observations(w, d0, kf, lmk)
        x1 = be.covariance_cross(0, kf, lmk, cam, meas)
        d1, t1 = be.get_deltas(0), be.get_trace(0)
        c1 = be.covariance(0, kf=[0, 1, 2], pairs=[(0, 1)], lmk="all")
        x2 = be.covariance_cross(0, kf, lmk, cam, meas)
        x3 = be.covariance_cross(0, kf, lmk)                                            # cross blocks only
    finally:
        be.close()
    for k in d0:
        assert d0[k].tobytes() == d1[k].tobytes(), k
    assert t0.tobytes() == t1.tobytes()
    for k in ("kf", "pair", "lmk"):
        assert c0[k].tobytes() == c1[k].tobytes(), k
    for k in ("cross", "innov", "maha2", "status"):
        assert x1[k].tobytes() == x2[k].tobytes(), k
    assert x3["cross"].tobytes() == x1["cross"].tobytes()
    assert np.all(x3["status"] == np.where(lmk == ch.SINGLE, xh.CROSS_LMK_SINGULAR, xh.CROSS_OK))


def test_window_2_of_a_batch_behind_decoys(backend_cls):
    """[decoy a, decoy b, pixel_vo]: the call at window index 2 within the bar at its own deltas, and — where the two solves return
    the same bits — the bits of the call on the window alone."""
    w = ch.window_pixel_vo()
    kf, lmk = xh.CASES["pixel_vo"][2](w)
    outs = []
    for ws, idx in (([w], 0), ([bt.decoy(bt.PIXEL, "a"), bt.decoy(bt.PIXEL, "b"), w], 2)):
        be = backend_cls(device=0)
        try:
            be.set_windows(ws); be.solve(_opts())
            d = be.get_deltas(idx)
            cam, meas = xh.candidate_observations(w, d, kf, lmk)
            got = be.covariance_cross(idx, kf, lmk, cam, meas)
        finally:
            be.close()
        _check("pixel_vo", w, d, kf, lmk, cam, meas, got, label=f" [window {idx} of {len(ws)}]")
        outs.append((d, got))
    same = all(outs[0][0][k].tobytes() == outs[1][0][k].tobytes() for k in outs[0][0])
    print(f"[cov cross] window 2 behind decoys: deltas bit-identical to the window alone: {same}")
    if same:
        for k in ("cross", "innov", "maha2", "status"):
            assert outs[0][1][k].tobytes() == outs[1][1][k].tobytes(), k
