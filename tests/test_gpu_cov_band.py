"""The band route of sadvio_ba_covariance / sadvio_ba_covariance_batch (cov_band_kernels.h) on the device, against the float64 inverse
of the FULL information matrix (cov_helpers.Information, evaluated at the deltas the device's own solve returned) and, for the
window of 2 064 columns, against the block-sparse Schur reference of cov_band_helpers. A device block passes when its relative
difference (cov_helpers.rel_diff) is at most TOL_FACTOR = 64 x E_REF of its window (cov_band_helpers.E_REF, measured by
tests/test_cov_band_cpu.py against 50 digits). Every test prints its worst figure before it asserts. Every test but the last forces
the route with SADVIO_COV_BAND=1 (read when the handle is created); the last runs with no variable set."""
import dataclasses

import numpy as np
import pytest

import cov_band_helpers as cb
import cov_helpers as ch
from sadvio_amd import capi, synthetic

pytestmark = pytest.mark.gpu
BAND, DENSE, LDS = capi.COV_ROUTE_BAND, capi.COV_ROUTE_DENSE, capi.COV_ROUTE_LDS


@pytest.fixture
def band_on(monkeypatch):
    monkeypatch.setenv("SADVIO_COV_BAND", "1")


def _opts(huber=0.0, iters=None):
    o = capi.reference_options()
    o.huber_a = huber
    if iters is not None:
        o.max_num_iterations = iters
    return o


def _pairs(w):
    """Every in-band pair and the two outermost free key-frames in both orders (outside the band)."""
    hb, _, _ = cb.bandwidth(w)
    f = cb.free_index(w)
    free = [k for k in range(w.n_kf) if f[k] >= 0]
    far = [(free[0], free[-1]), (free[-1], free[0])]
    assert abs(f[far[0][0]] - f[far[0][1]]) > hb
    return cb.in_band_pairs(w, hb) + far


def _solve_cov(backend_cls, w, opts, pairs, profile=False):
    be = backend_cls(device=0, profile_kernels=profile)
    try:
        be.set_windows([w])
        be.solve(opts)
        d = be.get_deltas(0)
        c = be.covariance(0, kf=list(range(w.n_kf)), pairs=list(pairs), lmk="all")
        times = be.kernel_times() if profile else None
    finally:
        be.close()
    return d, c, times


def _check(case, w, d, c, huber=0.0, pairs=()):
    info = ch.Information(w, d, huber)
    ref = ch.reference_blocks(info)
    tol = ch.TOL_FACTOR * cb.E_REF[case]
    worst = {"kf": 0.0, "pair": 0.0, "lmk": 0.0}
    for k in range(w.n_kf):
        worst["kf"] = max(worst["kf"], ch.rel_diff(c["kf"][k], ref["kf"][k]))
    for i, (a, b) in enumerate(pairs):
        worst["pair"] = max(worst["pair"], ch.rel_diff(c["pair"][i], ref["cross"](a, b)))
    for l in range(w.n_lmk):
        if l in info.singular:
            assert np.isnan(c["lmk"][l]).all(), l
        else:
            assert np.isfinite(c["lmk"][l]).all(), l
            worst["lmk"] = max(worst["lmk"], ch.rel_diff(c["lmk"][l], ref["lmk"][l]))
    print(f"[cov band] {case}: worst relative block difference kf {worst['kf']:.3e} pair {worst['pair']:.3e} lmk {worst['lmk']:.3e}; "
          f"bound {tol:.3e} (64 x e_ref {cb.E_REF[case]:.1e})")
    assert c["n_lmk_singular"] == len(info.singular)
    assert max(worst.values()) <= tol, (case, worst, tol)
    return info, ref


def _case(backend_cls, case, profile=False):
    build, huber = cb.WINDOWS[case]
    w = build()
    pairs = _pairs(w)
    d, c, times = _solve_cov(backend_cls, w, _opts(huber), pairs, profile)
    _check(case, w, d, c, huber, pairs)
    return w, pairs, d, c, times


def test_pixel_vo_across_several_band_steps(backend_cls, band_on):
    """N_p = 66, bw = 30: all key-frame blocks, every in-band pair, the pairs (0, 10) and (10, 0) outside the band, all landmarks.
    On a profiling handle the route shows as the class cov_band, and cov_invert has no launch."""
    w, pairs, d, c, times = _case(backend_cls, "vo12", profile=True)
    assert cb.bandwidth(w)[:2] == (4, 30) and pairs[-2:] == [(0, 10), (10, 0)]
    assert np.array_equal(c["pair"][-2], c["pair"][-1].T)                         # the canonical block and its exact transpose
    assert np.all(c["kf"][11] == 0.0)                                             # the constant key-frame
    assert times["cov_band"]["launches"] >= 1 and times["cov_band_sel"]["launches"] >= 1 and "cov_invert" not in times, sorted(times)
    for k in range(11):
        assert np.array_equal(c["kf"][k], c["kf"][k].T) and np.all(np.linalg.eigvalsh(c["kf"][k]) > 0)


def test_angular_variant(backend_cls, band_on):
    _case(backend_cls, "vo12_angular")


def test_window_whose_image_slides_and_whose_solve_is_out_of_lds(backend_cls, band_on):
    """N_p = 234 (the solve's HBM-resident path), bw = 54: the 60-column LDS image slides 39 block columns."""
    w, _, _, _, _ = _case(backend_cls, "vo40")
    assert 6 * int((w.kf_const == 0).sum()) == 234 and cb.bandwidth(w)[1] == 54


def test_vio_chain_with_imu_pairs(backend_cls, band_on):
    """dpf = 15, block columns of 5; 15 x 15 blocks."""
    w, _, _, c, _ = _case(backend_cls, "vio8")
    assert c["kf"].shape == (8, 15, 15) and w.has_imu and len(w.imu_factors) == 7


def test_relative_pose_factor_widens_the_band(backend_cls, band_on):
    """One SADVIO_SPARSE_RELATIVE_POSE factor between key-frames further apart than any landmark couples: the route must take
    bw = 48, not the landmarks' 30 (with 30 the factor's block of S would be cut off and every block would miss the bar)."""
    w, _, _, _, _ = _case(backend_cls, "relpose")
    assert cb.bandwidth(w)[1] == 48 and cb.bandwidth(cb.window_vo12())[1] == 30


def test_huber(backend_cls, band_on):
    w, pairs, _, c, _ = _case(backend_cls, "huber")
    _, c0, _ = _solve_cov(backend_cls, w, _opts(), pairs)
    assert ch.rel_diff(c["kf"][0], c0["kf"][0]) > 1e-3                             # the corrector is really applied


# ---- contract ---------------------------------------------------------------------------------------------------------------------
def test_two_calls_identical_and_solve_results_untouched(backend_cls, band_on):
    w = cb.window_vo12()
    pairs = [(0, 1), (0, 10), (10, 0), (2, 9)]
    be = backend_cls(device=0)
    try:
        be.set_windows([w])
        be.solve(_opts())
        d0, t0 = be.get_deltas(0), be.get_trace(0)
        c1 = be.covariance(0, kf=list(range(12)), pairs=pairs, lmk="all")
        d1, t1 = be.get_deltas(0), be.get_trace(0)
        c2 = be.covariance(0, kf=list(range(12)), pairs=pairs, lmk="all")
        c3 = be.covariance(0, pairs=[(10, 0)], lmk=[5, 5])                       # a pair's bits do not depend on what else is asked for
    finally:
        be.close()
    for k in d0:
        assert d0[k].tobytes() == d1[k].tobytes(), k
    assert t0.tobytes() == t1.tobytes()
    for k in ("kf", "pair", "lmk"):
        assert c1[k].tobytes() == c2[k].tobytes(), k
    assert c3["pair"][0].tobytes() == c1["pair"][2].tobytes() and c3["lmk"][0].tobytes() == c1["lmk"][5].tobytes() == c3["lmk"][1].tobytes()
    assert np.array_equal(c1["pair"][1], c1["pair"][2].T)


def test_unanchored_chain_is_not_usable(backend_cls, band_on):
    """No constant key-frame, no prior: a pivot of the band factor fails its test; a return code, the outputs untouched. The batch
    call reports it per item, on the same route."""
    w = synthetic.make_window(n_kf=12, n_lmk=200, length=6.0, band=3, seed=3, fixed=0)
    w.pose_priors = []
    be = backend_cls(device=0)
    try:
        be.set_windows([w]); be.solve(_opts())
        r = be.covariance(0, kf=[0, 1], pairs=[(0, 1), (0, 11)], lmk="all", raw_rc=True)
        b = be.covariance_batch([dict(w=0, kf=[0, 1], pairs=[(0, 11)], lmk="all")], fill=7.5)[0]
    finally:
        be.close()
    assert r["rc"] == capi.E_NOT_USABLE and "positive definite" in r["error"]
    assert np.all(r["kf"] == 0.0) and np.all(r["pair"] == 0.0) and np.all(r["lmk"] == 0.0)
    assert b["status"] == capi.E_NOT_USABLE and b["route"] == BAND
    assert np.all(b["kf"] == 7.5) and np.all(b["pair"] == 7.5) and np.all(b["lmk"] == 7.5)


def test_window_with_a_resident_dense_prior_keeps_the_dense_route(backend_cls, band_on):
    """A dense prior fills S: bw = N_p, not bandable, whatever the variable says (tests/test_gpu_cov.py's VIO window)."""
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
    assert times["cov_invert"]["launches"] >= 1 and "cov_band" not in times, sorted(times)
    assert b["route"] == LDS
    info = ch.Information(w_ref, d, 0.0)
    ref = ch.reference_blocks(info)
    assert max(ch.rel_diff(c["kf"][k], ref["kf"][k]) for k in range(4)) <= ch.TOL_FACTOR * ch.E_REF["vio_dense"]


def test_band_0_gives_the_dense_routes_bits_and_the_routes_agree(backend_cls, monkeypatch):
    """SADVIO_COV_BAND=0 and the unset variable both take the dense route on this window (N_p = 66 is served by it); 1 takes the band
    route. Two handles do not solve to the same bits (the solve's own sums are not ordered, tests/test_gpu_cov_batch.py::
    test_groups), so every run is held to the bar at its own deltas, bits are compared where the deltas are bit-identical, and the
    band run lies within the bar of the dense run where the state is the same — within the sum of the two bars otherwise, each run
    being within one bar of the reference at its own state and the states apart by the solve's rounding."""
    w = cb.window_vo12()
    pairs = _pairs(w)
    got = {}
    for val in (None, "0", "1"):
        if val is None:
            monkeypatch.delenv("SADVIO_COV_BAND", raising=False)
        else:
            monkeypatch.setenv("SADVIO_COV_BAND", val)
        got[val] = _solve_cov(backend_cls, w, _opts(), pairs, profile=True)
        _check("vo12", w, got[val][0], got[val][1], pairs=pairs)
    (d0, c0, t0), (dz, cz, tz), (d1, c1, t1) = got[None], got["0"], got["1"]
    assert "cov_invert" in t0 and "cov_band" not in t0 and "cov_invert" in tz and "cov_band" not in tz
    assert "cov_band" in t1 and "cov_invert" not in t1
    same_z = all(d0[k].tobytes() == dz[k].tobytes() for k in d0)
    same_1 = all(d0[k].tobytes() == d1[k].tobytes() for k in d0)
    worst_z = max([ch.rel_diff(a, b) for key in ("kf", "pair", "lmk") for a, b in zip(cz[key], c0[key])])
    worst_1 = max([ch.rel_diff(a, b) for key in ("kf", "pair", "lmk") for a, b in zip(c1[key], c0[key])])
    bar = ch.TOL_FACTOR * cb.E_REF["vo12"]
    print(f"[cov band] against the unset run: SADVIO_COV_BAND=0 {worst_z:.3e} (deltas bit-identical {same_z}); =1 {worst_1:.3e} "
          f"(deltas bit-identical {same_1}); bar {bar:.3e}")
    if same_z:
        assert all(c0[k].tobytes() == cz[k].tobytes() for k in ("kf", "pair", "lmk"))
    assert worst_z <= 2 * bar
    assert 0.0 < worst_1 <= (bar if same_1 else 2 * bar)


# ---- batch ------------------------------------------------------------------------------------------------------------------------
def test_batch_reports_the_route_and_returns_the_single_calls_bits(backend_cls, band_on):
    """Bandable windows report BAND and return the single call's bits, whatever else the call holds; a window whose band is the whole
    of S (two free key-frames that share landmarks: bw = N_p) is not bandable and keeps its LDS route under SADVIO_COV_BAND=1."""
    ws = [cb.window_vo12(), ch.window_pixel_vo(), cb.window_vo40()]
    items = [dict(w=0, kf=list(range(12)), pairs=[(0, 1), (0, 10), (10, 0)], lmk="all"), dict(w=1, kf=[0, 1], lmk="all"),
             dict(w=2, kf=[0, 20, 38], pairs=[(0, 38), (5, 7)], lmk=[3, 4]), dict(w=0, kf=[4], pairs=[(10, 0)])]
    be = backend_cls(device=0)
    try:
        be.set_windows(ws)
        be.solve(_opts())
        got = be.covariance_batch(items)
        single = [be.covariance(it["w"], kf=it.get("kf"), pairs=it.get("pairs"), lmk=it.get("lmk")) for it in items]
    finally:
        be.close()
    assert [g["route"] for g in got] == [BAND, LDS, BAND, BAND] and all(g["status"] == 0 for g in got)
    for g, s in zip(got, single):
        if g["route"] != BAND:
            continue
        for k in ("kf", "pair", "lmk"):
            assert g[k].tobytes() == s[k].tobytes(), k
        assert g["n_lmk_singular"] == s["n_lmk_singular"]
    assert got[3]["pair"][0].tobytes() == got[0]["pair"][2].tobytes()


def test_batch_after_the_throughput_kernels(backend_cls, band_on, monkeypatch):
    """A batch k_lm_pass solved (the single call refuses it): route BAND, and the blocks pass the bar at get_deltas' deltas."""
    monkeypatch.setenv("SADVIO_LM", "1")
    w = cb.window_vo12()
    pairs = _pairs(w)
    be = backend_cls(device=0, profile_kernels=True)
    try:
        be.set_windows([w])
        be.solve(_opts())
        times = be.kernel_times()
        d = be.get_deltas(0)
        r = be.covariance(0, kf=[0], raw_rc=True)
        got = be.covariance_batch([dict(w=0, kf=list(range(12)), pairs=pairs, lmk="all")])[0]
    finally:
        be.close()
    assert "k_lm_pass" in times and "k_backsub" not in times, sorted(times)
    assert r["rc"] == capi.E_INVALID_ARG and "throughput" in r["error"]
    assert got["route"] == BAND and got["status"] == 0
    _check("vo12", w, d, got, pairs=pairs)


# ---- the default route at size ----------------------------------------------------------------------------------------------------
def test_default_route_at_2064_columns(backend_cls, monkeypatch):
    """No variable set. 345 key-frames, 344 free: N_p = 2 064, which the dense route refuses. The call is accepted, the route is
    BAND; the first, middle and last key-frame block, a pair inside the band, a pair outside it in both orders and 20 landmark
    blocks against the Schur reference at the device's own deltas."""
    monkeypatch.delenv("SADVIO_COV_BAND", raising=False)
    w = cb.window_at_size()
    hb, bw, _ = cb.bandwidth(w)
    kf, pairs, lmk = cb.at_size_request(w, hb)
    be = backend_cls(device=0, profile_kernels=True)
    try:
        be.set_windows([w])
        be.solve(_opts())
        d = be.get_deltas(0)
        c = be.covariance(0, kf=kf, pairs=pairs, lmk=lmk)
        times = be.kernel_times()
        b = be.covariance_batch([dict(w=0, kf=kf, pairs=pairs, lmk=lmk)])[0]
    finally:
        be.close()
    assert 6 * int((w.kf_const == 0).sum()) == 2064
    assert b["route"] == BAND and b["status"] == 0
    assert times["cov_band"]["launches"] >= 1 and "cov_invert" not in times, sorted(times)
    for k in ("kf", "pair", "lmk"):
        assert b[k].tobytes() == c[k].tobytes(), k
    assert np.array_equal(c["pair"][1], c["pair"][2].T)
    ref = cb.SchurBlocks(w, d).blocks(kf, pairs, lmk)
    worst = {k: max(ch.rel_diff(a, r) for a, r in zip(c[k], ref[k])) for k in ("kf", "pair", "lmk")}
    tol = ch.TOL_FACTOR * cb.E_REF["at_size"]
    print(f"[cov band] at_size: N_p 2064, hb {hb}, bw {bw}: worst relative block difference kf {worst['kf']:.3e} pair {worst['pair']:.3e} "
          f"lmk {worst['lmk']:.3e}; bound {tol:.3e} (64 x e_ref {cb.E_REF['at_size']:.1e})")
    assert c["n_lmk_singular"] == 0 and np.isfinite(c["lmk"]).all()
    assert max(worst.values()) <= tol, (worst, tol)
