"""The border route of sadvio_ba_covariance / sadvio_ba_covariance_batch (cov_border_kernels.h, cov_border_plan.h) on the device: long
windows whose loop closures keep S from being banded. Against the float64 inverse of the FULL information matrix
(cov_helpers.Information at the deltas the device's own solve returned) and, for the window of 2 064 columns, against the
block-sparse Schur reference (cov_border_helpers.schur_blocks). A device block passes when its relative difference
(cov_helpers.rel_diff) is at most TOL_FACTOR = 64 x E_REF of its window (cov_border_helpers.E_REF, measured by
tests/test_cov_border_cpu.py against 50 digits). Every test prints its worst figure before it asserts.

Every test but the last runs with SADVIO_COV_BAND=1, SADVIO_COV_BORDER=1 and SADVIO_COV_BORDER_HB lowered (all read when the handle
is created) so that windows of 8 to 40 key-frames have closure edges; the last runs with no variable set.

hb_lim of window_vo12's cases: the window's own landmarks couple free key-frames up to 4 apart, so SADVIO_COV_BORDER_HB=4 is the
value at which the relative-pose factor is the only closure edge and the border is one key-frame ("closure12"); at 3 two landmark
couplings are closure edges too and the border is two key-frames ("closure12_hb3"). Both run.

The two pivot refusals: in an unanchored chain the core stays positive definite (holding the border key-frame fixes the gauge), so
that refusal is the test on T; a window whose floating half lies wholly in the core fails a pivot of B."""
import numpy as np
import pytest

import cov_band_helpers as cb
import cov_border_helpers as bh
import cov_helpers as ch
from sadvio_amd import capi, synthetic

pytestmark = pytest.mark.gpu
BORDER, BAND, DENSE, LDS = capi.COV_ROUTE_BORDER, capi.COV_ROUTE_BAND, capi.COV_ROUTE_DENSE, capi.COV_ROUTE_LDS
NEW_CLASSES = ("cov_border_split", "cov_border_solve", "cov_border_schur", "cov_border_apply")


def _env(monkeypatch, hb, band="1", border="1"):
    for name, val in (("SADVIO_COV_BAND", band), ("SADVIO_COV_BORDER", border), ("SADVIO_COV_BORDER_HB", None if hb is None else str(hb))):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, val)


def _opts(huber=0.0):
    o = capi.reference_options()
    o.huber_a = huber
    return o


def _solve_cov(backend_cls, w, opts, pairs, profile=False, **flags):
    be = backend_cls(device=0, profile_kernels=profile, **flags)
    try:
        be.set_windows([w])
        be.solve(opts)
        d = be.get_deltas(0)
        c = be.covariance(0, kf=list(range(w.n_kf)), pairs=list(pairs), lmk="all")
        times = be.kernel_times() if profile else None
    finally:
        be.close()
    return d, c, times


def _check(case, w, d, c, kinds, huber=0.0):
    info = ch.Information(w, d, huber)
    ref = ch.reference_blocks(info)
    tol = ch.TOL_FACTOR * bh.E_REF[case]
    worst = {"kf": 0.0, "lmk": 0.0}
    for k in range(w.n_kf):
        worst["kf"] = max(worst["kf"], ch.rel_diff(c["kf"][k], ref["kf"][k]))
    i = 0
    for kind, pairs in kinds.items():
        worst[kind] = 0.0
        for (a, b) in pairs:
            worst[kind] = max(worst[kind], ch.rel_diff(c["pair"][i], ref["cross"](a, b)))
            i += 1
    for l in range(w.n_lmk):
        if l in info.singular:
            assert np.isnan(c["lmk"][l]).all(), l
        else:
            assert np.isfinite(c["lmk"][l]).all(), l
            worst["lmk"] = max(worst["lmk"], ch.rel_diff(c["lmk"][l], ref["lmk"][l]))
    print(f"[cov border] {case}: worst relative block difference " + " ".join(f"{k} {v:.3e}" for k, v in worst.items()) +
          f"; bound {tol:.3e} (64 x e_ref {bh.E_REF[case]:.1e})")
    assert c["n_lmk_singular"] == len(info.singular)
    assert max(worst.values()) <= tol, (case, worst, tol)
    return ref


def _case(backend_cls, monkeypatch, case, profile=True, **flags):
    build, huber, hb = bh.WINDOWS[case]
    _env(monkeypatch, hb)
    w = build()
    plan = bh.plan_of(w, hb)
    assert plan.answer == "OK" and plan.hb_core <= hb
    kinds = bh.request_pairs(w, plan, every=len(plan.core_of) <= 16)
    d, c, times = _solve_cov(backend_cls, w, _opts(huber), bh.flat_pairs(kinds), profile, **flags)
    if profile:
        assert all(times[k]["launches"] >= 1 for k in NEW_CLASSES + ("cov_band", "cov_band_sel")) and "cov_invert" not in times, sorted(times)
    _check(case, w, d, c, kinds, huber)
    n_far = len(kinds["far"])
    assert np.array_equal(c["pair"][-n_far], c["pair"][-1].T)                      # the block outside the core band and its exact transpose
    return w, plan, kinds, d, c


# ---- accuracy ---------------------------------------------------------------------------------------------------------------------
def test_one_closure_factor_gives_a_border_of_one(backend_cls, monkeypatch):
    """window_vo12 plus window_relpose's factor between key-frames 1 and 8: N_p = 66, border {1}, core of 10 key-frames with
    hb' = 4 (bw' = 30, the image of 36 columns slides over the 60 core columns)."""
    w, plan, kinds, _, c = _case(backend_cls, monkeypatch, "closure12")
    assert plan.border == [1] and plan.hb_core == 4 and len(kinds["cross"]) == 20
    assert np.all(c["kf"][11] == 0.0)                                             # the constant key-frame
    for k in range(11):
        assert np.array_equal(c["kf"][k], c["kf"][k].T) and np.all(np.linalg.eigvalsh(c["kf"][k]) > 0)


def test_hb_lim_3_takes_two_landmark_couplings_into_the_border_too(backend_cls, monkeypatch):
    w, plan, kinds, _, _ = _case(backend_cls, monkeypatch, "closure12_hb3")
    assert plan.border == [1, 2] and plan.hb_core == 3 and len(kinds["bb"]) == 2


def test_landmark_seen_again_from_the_other_end(backend_cls, monkeypatch):
    """One landmark observed from key-frames 0, 1, 2 and 8, 9, 10: nine closure edges, a border of three (not six), and that
    landmark's block is formed from Sigma_BD and Sigma_DD as well as the core band."""
    w, plan, kinds, d, c = _case(backend_cls, monkeypatch, "revisit12")
    k = set(w.obs_kf[w.lmk_obs_ptr[bh.REVISIT_LMK]:w.lmk_obs_ptr[bh.REVISIT_LMK + 1]].tolist())
    assert k == {0, 1, 2, 8, 9, 10} and plan.border == [0, 1, 2] and plan.n_edges == 9
    info = ch.Information(w, d, 0.0)
    e = ch.rel_diff(c["lmk"][bh.REVISIT_LMK], ch.reference_blocks(info)["lmk"][bh.REVISIT_LMK])
    print(f"[cov border] revisit12: the re-observed landmark's block {e:.3e}")
    assert e <= ch.TOL_FACTOR * bh.E_REF["revisit12"]


def test_core_over_several_block_columns_and_solve_out_of_lds(backend_cls, monkeypatch):
    """window_vo40 with a factor between key-frames 3 and 33: N_p = 234, the core has 228 columns and bw' = 48, so the 54-column
    image slides over 30 block columns and the substitutions of k_cov_border_solve run past their LDS window."""
    w, plan, _, _, _ = _case(backend_cls, monkeypatch, "closure40")
    assert plan.border == [3] and plan.n_core == 38 and plan.hb_core == 7


def test_vio_chain_with_a_closure(backend_cls, monkeypatch):
    """dpf = 15, block columns of 5, 15 right-hand sides in k_cov_border_solve's workgroup. The closure is a landmark seen from
    key-frames 0 and 6: set_sparse_priors refuses a relative-pose factor on a window that carries IMU states."""
    w, plan, _, _, c = _case(backend_cls, monkeypatch, "closure_vio8")
    assert c["kf"].shape == (8, 15, 15) and plan.border == [0] and plan.hb_core == 2


def test_angular_variant(backend_cls, monkeypatch):
    _case(backend_cls, monkeypatch, "closure12_angular", profile=False)


def test_huber(backend_cls, monkeypatch):
    w, _, kinds, _, c = _case(backend_cls, monkeypatch, "closure12_huber", profile=False)
    _, c0, _ = _solve_cov(backend_cls, w, _opts(), bh.flat_pairs(kinds))
    assert ch.rel_diff(c["kf"][0], c0["kf"][0]) > 1e-3                             # the corrector is really applied


# ---- pivot tests, repeatability, side effects -------------------------------------------------------------------------------------
def test_unanchored_chain_is_not_usable(backend_cls, monkeypatch):
    """No constant key-frame, no pose prior, one closure factor: the core is positive definite, T is not; a return code, the outputs
    untouched. The batch call reports it per item, on the same route."""
    _env(monkeypatch, 4)
    w = synthetic.make_window(n_kf=12, n_lmk=200, length=6.0, band=3, seed=3, fixed=0)
    w.pose_priors = []
    w = bh.add_relpose(w, *cb.RELPOSE_KF)
    assert bh.plan_of(w, 4).border == [1]
    be = backend_cls(device=0)
    try:
        be.set_windows([w]); be.solve(_opts())
        r = be.covariance(0, kf=[0, 1], pairs=[(0, 1), (0, 11)], lmk="all", raw_rc=True)
        b = be.covariance_batch([dict(w=0, kf=[0, 1], pairs=[(0, 11)], lmk="all")], fill=7.5)[0]
    finally:
        be.close()
    assert r["rc"] == capi.E_NOT_USABLE and "positive definite" in r["error"]
    assert np.all(r["kf"] == 0.0) and np.all(r["pair"] == 0.0) and np.all(r["lmk"] == 0.0)
    assert b["status"] == capi.E_NOT_USABLE and b["route"] == BORDER
    assert np.all(b["kf"] == 7.5) and np.all(b["pair"] == 7.5) and np.all(b["lmk"] == 7.5)


def test_floating_half_in_the_core_is_not_usable(backend_cls, monkeypatch):
    """cov_border_helpers.window_floating_half: the gauge freedom sits in the core, a pivot of B fails in k_cov_band_chol, and
    the kernels behind it leave everything as it is: a return code, the outputs untouched."""
    _env(monkeypatch, 3)
    w = bh.window_floating_half()
    plan = bh.plan_of(w, 3)
    assert plan.answer == "OK" and min(plan.border) >= 6
    be = backend_cls(device=0, profile_kernels=True)
    try:
        be.set_windows([w]); be.solve(_opts())
        r = be.covariance(0, kf=[0, 7], pairs=[(0, 1), (0, 9), (plan.border[0], 0)], lmk="all", raw_rc=True)
        times = be.kernel_times()
    finally:
        be.close()
    assert all(k in times for k in NEW_CLASSES), sorted(times)
    assert r["rc"] == capi.E_NOT_USABLE and "positive definite" in r["error"]
    assert np.all(r["kf"] == 0.0) and np.all(r["pair"] == 0.0) and np.all(r["lmk"] == 0.0)


def test_two_calls_identical_solve_untouched_and_batch_returns_the_same_bits(backend_cls, monkeypatch):
    _env(monkeypatch, 4)
    w = bh.window_revisit12()
    pairs = [(0, 1), (1, 0), (3, 4), (3, 10), (10, 3), (0, 9), (9, 0), (5, 6)]     # border x border, core band, core outside the band, border x core
    be = backend_cls(device=0)
    try:
        be.set_windows([w])
        be.solve(_opts())
        d0, t0 = be.get_deltas(0), be.get_trace(0)
        c1 = be.covariance(0, kf=list(range(12)), pairs=pairs, lmk="all")
        d1, t1 = be.get_deltas(0), be.get_trace(0)
        c2 = be.covariance(0, kf=list(range(12)), pairs=pairs, lmk="all")
        c3 = be.covariance(0, pairs=[(10, 3)], lmk=[5, 5])                        # a pair's bits do not depend on what else is asked for
        b = be.covariance_batch([dict(w=0, kf=list(range(12)), pairs=pairs, lmk="all"), dict(w=0, pairs=[(10, 3)])])
    finally:
        be.close()
    for k in d0:
        assert d0[k].tobytes() == d1[k].tobytes(), k
    assert t0.tobytes() == t1.tobytes()
    for k in ("kf", "pair", "lmk"):
        assert c1[k].tobytes() == c2[k].tobytes(), k
        assert b[0][k].tobytes() == c1[k].tobytes(), k
    assert [g["route"] for g in b] == [BORDER, BORDER] and all(g["status"] == 0 for g in b)
    assert b[1]["pair"][0].tobytes() == c1["pair"][4].tobytes() == c3["pair"][0].tobytes()
    assert c3["lmk"][0].tobytes() == c1["lmk"][5].tobytes() == c3["lmk"][1].tobytes()
    for i in (0, 3, 5):
        assert np.array_equal(c1["pair"][i], c1["pair"][i + 1].T), pairs[i]
    assert np.abs(c1["pair"]).min(axis=(1, 2)).max() > 0.0


# ---- route selection --------------------------------------------------------------------------------------------------------------
def test_border_0_and_unset_keep_the_dense_route(backend_cls, monkeypatch):
    """SADVIO_COV_BORDER=0 and the unset variable both leave this window (N_p = 66) on the route it had; 1 takes the border route.
    Two handles do not solve to the same bits (tests/test_gpu_cov_band.py says why), so every run is held to the bar at its own
    deltas and bits are compared where the deltas are bit-identical."""
    w = cb.window_relpose()
    plan = bh.plan_of(w, 4)
    kinds = bh.request_pairs(w, plan)
    got = {}
    for val in (None, "0", "1"):
        _env(monkeypatch, 4, band=None, border=val)
        got[val] = _solve_cov(backend_cls, w, _opts(), bh.flat_pairs(kinds), profile=True)
        _check("closure12", w, got[val][0], got[val][1], kinds)
    (d0, c0, t0), (dz, cz, tz), (d1, c1, t1) = got[None], got["0"], got["1"]
    for t in (t0, tz):
        assert "cov_invert" in t and "cov_band" not in t and not any(k in t for k in NEW_CLASSES), sorted(t)
    assert all(k in t1 for k in NEW_CLASSES) and "cov_invert" not in t1
    if all(d0[k].tobytes() == dz[k].tobytes() for k in d0):
        assert all(c0[k].tobytes() == cz[k].tobytes() for k in ("kf", "pair", "lmk"))
    # with the band route forced and the border route off, the window takes the band route as before (bw = 48)
    _env(monkeypatch, 4, band="1", border="0")
    _, _, tb = _solve_cov(backend_cls, w, _opts(), bh.flat_pairs(kinds), profile=True)
    assert "cov_band" in tb and not any(k in tb for k in NEW_CLASSES)


def test_long_track_across_the_closure(backend_cls, monkeypatch):
    """SADVIO_LONG_MIN=6 makes the re-observed landmark of window_revisit12 (six observations, every other landmark has five) a long
    track: k_cov_long assembles it, k_cov_lmk_long reads Sigma at pairs that touch the border."""
    monkeypatch.setenv("SADVIO_LONG_MIN", "6")
    w, plan, _, _, _ = _case(backend_cls, monkeypatch, "revisit12", long_tracks=True, long_track_covariance=True)
    assert int((np.diff(w.lmk_obs_ptr) >= 6).sum()) == 1


# ---- refusals keep their texts ----------------------------------------------------------------------------------------------------
def test_covariance_cross_keeps_the_route_it_had(backend_cls, monkeypatch):
    """sadvio_ba_covariance_cross does not take the border route: under SADVIO_COV_BORDER=1 this window is served as before (the
    band route, SADVIO_COV_BAND=1), with the bits of a handle on which the border route is off."""
    w = cb.window_relpose()
    out = {}
    for val in ("1", "0"):
        _env(monkeypatch, 4, border=val)
        be = backend_cls(device=0, profile_kernels=True)
        try:
            be.set_windows([w]); be.solve(_opts())
            d = be.get_deltas(0)
            x = be.covariance_cross(0, kf=[0, 1, 8], lmk=[3, 50, 150])
            out[val] = (d, x, be.kernel_times())
        finally:
            be.close()
    assert not any(k in out["1"][2] for k in NEW_CLASSES) and "cov_band" in out["1"][2]
    if all(out["1"][0][k].tobytes() == out["0"][0][k].tobytes() for k in out["1"][0]):
        assert out["1"][1]["cross"].tobytes() == out["0"][1]["cross"].tobytes()


def test_border_wider_than_96_columns_is_not_borderable(backend_cls, monkeypatch):
    """window_vo40 at hb_lim = 1: the landmarks' own couplings need far more than 16 border key-frames, the planner answers
    TOO_WIDE and the window keeps the band route SADVIO_COV_BAND=1 gives it."""
    _env(monkeypatch, 1)
    w = cb.window_vo40()
    assert bh.plan_of(w, 1).answer == "TOO_WIDE"
    _, _, times = _solve_cov(backend_cls, w, _opts(), [(0, 1)], profile=True)
    assert "cov_band" in times and not any(k in times for k in NEW_CLASSES)


def test_window_with_a_resident_dense_prior_keeps_the_dense_route(backend_cls, monkeypatch):
    """A dense prior fills S: not borderable, whatever the variables say (tests/test_gpu_cov.py's VIO window, as
    tests/test_gpu_cov_band.py runs it)."""
    import dataclasses
    _env(monkeypatch, 1)
    w, args, w2, keep = ch.vio_marg_step()
    be = backend_cls(device=0, profile_kernels=True)
    try:
        be.set_prior(ch.VIO_J0, np.zeros(15))
        be.set_windows([w])
        g = be.marginalize(0, form="cholesky", readback=True, **args)
        w_ref = ch.vio_attach(w, w2, keep, g, None)
        w_dev = dataclasses.replace(w_ref, dense_prior=dict({k: v for k, v in w_ref.dense_prior.items() if k not in ("J", "r0")}, resident=True))
        be.set_windows([w_dev])
        be.solve(_opts())
        d = be.get_deltas(0)
        c = be.covariance(0, kf=list(range(4)), pairs=[(0, 3)], lmk="all")
        times = be.kernel_times()
        b = be.covariance_batch([dict(w=0, kf=[0])])[0]
    finally:
        be.close()
    assert times["cov_invert"]["launches"] >= 1 and "cov_band" not in times and not any(k in times for k in NEW_CLASSES), sorted(times)
    assert b["route"] == LDS
    ref = ch.reference_blocks(ch.Information(w_ref, d, 0.0))
    assert max(ch.rel_diff(c["kf"][k], ref["kf"][k]) for k in range(4)) <= ch.TOL_FACTOR * ch.E_REF["vio_dense"]


# ---- the default route at size ----------------------------------------------------------------------------------------------------
def test_default_route_at_2064_columns_with_a_closure(backend_cls, monkeypatch):
    """No variable set. cov_band_helpers.window_at_size (345 key-frames, N_p = 2 064) plus one relative-pose factor between free
    key-frames 5 and 340: not bandable, and refused before the border route existed ("the reduced system has 2047 columns or
    more"). Now SADVIO_OK through the border route: border {5}, a core of 2 058 columns. The first, middle and last key-frame
    block and the border's, neighbour pairs in the core and across the border, the closure pair in both orders, a core pair
    outside the band in both orders and 20 landmark blocks against the Schur reference at the device's own deltas. The same
    window is still refused by sadvio_ba_covariance_cross, text unchanged."""
    _env(monkeypatch, None, band=None, border=None)
    w = bh.window_at_size_closure()
    plan = bh.plan_of(w)
    a, b = bh.AT_SIZE_CLOSURE_KF
    assert plan.answer == "OK" and plan.border == [a] and plan.hb_core <= 19
    kf, _, lmk = cb.at_size_request(w, plan.hb_core)
    kf = kf + [a, b]
    pairs = [(172, 173), (173, 172), (4, 6), (4, 5), (5, 6), (a, b), (b, a), (3, 339), (339, 3)]
    be = backend_cls(device=0, profile_kernels=True)
    try:
        be.set_windows([w])
        be.solve(_opts())
        d = be.get_deltas(0)
        r = be.covariance(0, kf=kf, pairs=pairs, lmk=lmk, raw_rc=True)
        times = be.kernel_times()
        x = be.covariance_cross(0, kf=[0], lmk=[3], raw_rc=True)
        bt = be.covariance_batch([dict(w=0, kf=kf, pairs=pairs, lmk=lmk)])[0] if r.get("rc", 0) == 0 else None
    finally:
        be.close()
    assert 6 * int((w.kf_const == 0).sum()) == 2064
    assert r.get("rc", 0) == 0, r.get("error")
    c = r
    assert all(times[k]["launches"] >= 1 for k in NEW_CLASSES) and "cov_invert" not in times, sorted(times)
    assert x["rc"] == capi.E_INVALID_ARG and "the reduced system has 2047 columns or more" in x["error"]
    assert bt["route"] == BORDER and bt["status"] == 0
    for k in ("kf", "pair", "lmk"):
        assert bt[k].tobytes() == c[k].tobytes(), k
    assert np.array_equal(c["pair"][5], c["pair"][6].T) and np.array_equal(c["pair"][7], c["pair"][8].T) and np.array_equal(c["pair"][0], c["pair"][1].T)
    ref = bh.schur_blocks(w, d).blocks(kf, pairs, lmk)
    worst = {k: max(ch.rel_diff(g, r_) for g, r_ in zip(c[k], ref[k])) for k in ("kf", "pair", "lmk")}
    tol = ch.TOL_FACTOR * bh.E_REF["at_size_closure"]
    print(f"[cov border] at_size_closure: N_p 2064, border {plan.border}, hb' {plan.hb_core}: worst relative block difference kf {worst['kf']:.3e} "
          f"pair {worst['pair']:.3e} lmk {worst['lmk']:.3e}; bound {tol:.3e} (64 x e_ref {bh.E_REF['at_size_closure']:.1e})")
    print("[cov border] at_size_closure kernel classes (us): " + ", ".join(f"{k} {times[k]['avg_us']:.0f}" for k in NEW_CLASSES + ("cov_band", "cov_band_sel")))
    assert c["n_lmk_singular"] == 0 and np.isfinite(c["lmk"]).all()
    assert max(worst.values()) <= tol, (worst, tol)
