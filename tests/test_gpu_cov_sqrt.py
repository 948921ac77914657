"""The square-root assembly of sadvio_ba_covariance / sadvio_ba_covariance_batch (cov_kernels.h: k_cov_assemble_sqrt,
k_cov_schur_sqrt, k_cov_lmk<G, true>; SADVIO_COV_SQRT) on the device.

Windows with a landmark 1 mm / 0.1 mm from a camera centre are held to the 50-digit blocks that tests/cov_sqrt_helpers.py forms from
the float64 Jacobian at the device's own deltas (cov_helpers.Information's float64 H has lost what is tested); the existing families
to cov_helpers' float64 inverse at their existing bars. A device block passes at TOL_FACTOR = 64 x E_REF of its window. Every test
prints its worst figure before it asserts. Handles are created after the environment is set: EnvCfg reads it once."""
import dataclasses

import numpy as np
import pytest

import batch_helpers as bh
import cov_band_helpers as cbh
import cov_helpers as ch
import cov_sqrt_helpers as sh
from sadvio_amd import capi, synthetic

pytestmark = pytest.mark.gpu

PAIRS = [(0, 1), (1, 0), (0, 4)]


def _opts(huber=0.0, frozen=False):
    """frozen: max_num_iterations = 0, the deltas stay exactly zero. Two handles do not solve to the same bits (the solve's own sums
    are not ordered, tests/test_gpu_cov_band.py), so wherever two handles' covariances are compared bit for bit, both are frozen at
    the state the window was built at; every bar is met after a full solve."""
    o = capi.reference_options()
    o.huber_a = huber
    if frozen:
        o.max_num_iterations = 0
    return o


def _zero(d):
    return all(not np.any(v) for v in d.values())


def _env(monkeypatch, sqrt=None, band=None):
    for key, val in (("SADVIO_COV_SQRT", sqrt), ("SADVIO_COV_BAND", band)):
        if val is None:
            monkeypatch.delenv(key, raising=False)
        else:
            monkeypatch.setenv(key, str(val))


def _solve_cov(backend_cls, w, opts=None, pairs=(), use_graph=False, want_kf=True, profile=False, raw_rc=False):
    be = backend_cls(device=0, use_graph=use_graph, profile_kernels=profile)
    try:
        be.set_windows([w])
        be.solve(opts or _opts())
        d = be.get_deltas(0)
        c = be.covariance(0, kf=list(range(w.n_kf)) if want_kf else None, pairs=list(pairs), lmk="all", raw_rc=raw_rc)
        times = be.kernel_times() if profile else None
    finally:
        be.close()
    return d, c, times


def _check_near(case, w, d, c, pairs=PAIRS, tag=""):
    """Every key-frame block, the pairs and every landmark block of c against the 50-digit blocks at the deltas d."""
    lin = sh.Lin(w, d)
    ref = sh.mp_blocks_from_J(w, d, lin=lin)
    tol = ch.TOL_FACTOR * sh.E_REF[case]
    m = sh.device_worst(c, ref, lin, pairs)
    print(f"[cov sqrt] {case}{tag}: worst relative block difference kf {m['kf']:.3e} pair {m['pair']:.3e} lmk {m['lmk']:.3e}; "
          f"bound {tol:.3e} (64 x e_ref {sh.E_REF[case]:.1e})")
    assert tol <= 1e-6
    assert c["n_lmk_singular"] == len(ref["singular"])
    assert max(m.values()) <= tol, (case, m, tol)
    return lin, ref


def _check_family(case, w, d, c, huber=0.0, pairs=(), want_kf=True, w_ref=None):
    """tests/test_gpu_cov.py's comparison: the float64 inverse of the full information matrix at the deltas d, 64 x cov_helpers.E_REF."""
    info = ch.Information(w_ref if w_ref is not None else w, d, huber)
    ref = ch.reference_blocks(info)
    tol = ch.TOL_FACTOR * ch.E_REF[case]
    worst = {"kf": 0.0, "pair": 0.0, "lmk": 0.0}
    if want_kf:
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
    print(f"[cov sqrt] {case}: worst relative block difference kf {worst['kf']:.3e} pair {worst['pair']:.3e} lmk {worst['lmk']:.3e}; "
          f"bound {tol:.3e} (64 x e_ref {ch.E_REF[case]:.1e})")
    assert c["n_lmk_singular"] == len(info.singular)
    assert max(worst.values()) <= tol, (case, worst, tol)
    return info


def _same(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in ("kf", "pair", "lmk"))


# ---- 1, 2: the near-camera landmark ------------------------------------------------------------------------------------------------
def test_landmark_at_a_tenth_of_a_millimetre_is_served_through_the_retry(backend_cls, monkeypatch):
    """Variable unset: the plain form's S is indefinite, the pivot tests refuse it, the call assembles again in square-root form.
    Before the square-root assembly this call returned SADVIO_E_NOT_USABLE."""
    _env(monkeypatch)
    w = sh.window_near(1e-4)
    d, c, times = _solve_cov(backend_cls, w, pairs=PAIRS, profile=True)
    assert c["rc"] == capi.SADVIO_OK
    _check_near("near_1e-4", w, d, c)
    assert "cov_assemble_sqrt" in times and "cov_assemble" in times, sorted(times)
    assert np.array_equal(c["pair"][0], c["pair"][1].T)
    for l in range(w.n_lmk):
        assert np.array_equal(c["lmk"][l], c["lmk"][l].T) and np.all(np.linalg.eigvalsh(c["lmk"][l]) >= 0.0), l


@pytest.mark.parametrize("noisy", [False, True])
def test_landmark_at_a_millimetre(backend_cls, monkeypatch, noisy):
    """SADVIO_COV_SQRT=1 is within the bar; unset, the plain form passes its pivot tests, so the call returns the bits of
    SADVIO_COV_SQRT=0 — with the plain form's error, which is printed (about 5e-4)."""
    case = "near_1e-3_noisy" if noisy else "near_1e-3"
    w = sh.window_near(1e-3, noisy)
    _env(monkeypatch, sqrt=1)
    d1, c1, t1 = _solve_cov(backend_cls, w, pairs=PAIRS, profile=True)
    lin, ref = _check_near(case, w, d1, c1)
    assert "cov_assemble_sqrt" in t1 and "cov_assemble" not in t1, sorted(t1)
    _env(monkeypatch)
    du, cu, tu = _solve_cov(backend_cls, w, pairs=PAIRS, profile=True)
    assert "cov_assemble" in tu and "cov_assemble_sqrt" not in tu, sorted(tu)
    lin_u = sh.Lin(w, du)
    m = sh.device_worst(cu, sh.mp_blocks_from_J(w, du, lin=lin_u), lin_u, PAIRS)
    print(f"[cov sqrt] {case}: the plain form's worst relative block difference kf {m['kf']:.3e} pair {m['pair']:.3e} lmk {m['lmk']:.3e}")
    fu =_solve_cov(backend_cls, w, _opts(frozen=True), pairs=PAIRS)
    _env(monkeypatch, sqrt=0)
    f0 = _solve_cov(backend_cls, w, _opts(frozen=True), pairs=PAIRS)
    assert _zero(fu[0]) and _zero(f0[0])
    assert _same(fu[1], f0[1]) and fu[1]["n_lmk_singular"] == f0[1]["n_lmk_singular"]


# ---- 3: the existing families under SADVIO_COV_SQRT=1 ------------------------------------------------------------------------------
def test_pixel_vo(backend_cls, monkeypatch):
    _env(monkeypatch, sqrt=1)
    w = ch.window_pixel_vo()
    d, c, _ = _solve_cov(backend_cls, w, pairs=[(0, 1), (1, 0)])
    info = _check_family("pixel_vo", w, d, c, pairs=[(0, 1), (1, 0)])
    assert info.singular == [ch.SINGLE] and c["n_lmk_singular"] == 1 and np.isnan(c["lmk"][ch.SINGLE]).all()
    assert np.all(c["kf"][2] == 0.0)
    assert np.array_equal(c["pair"][0], c["pair"][1].T)
    for k in range(2):
        assert np.array_equal(c["kf"][k], c["kf"][k].T) and np.all(np.linalg.eigvalsh(c["kf"][k]) > 0)


def test_angular_vo(backend_cls, monkeypatch):
    _env(monkeypatch, sqrt=1)
    w = ch.window_angular_vo()
    pairs = [(0, 1), (0, 2), (1, 2)]
    d, c, _ = _solve_cov(backend_cls, w, pairs=pairs)
    _check_family("angular_vo", w, d, c, pairs=pairs)


def test_huber(backend_cls, monkeypatch):
    _env(monkeypatch, sqrt=1)
    w = ch.window_huber()
    d, c, _ = _solve_cov(backend_cls, w, _opts(ch.HUBER_A), pairs=[(0, 1)])
    _check_family("huber", w, d, c, huber=ch.HUBER_A, pairs=[(0, 1)])


@pytest.mark.parametrize("form", ["dense", "sparse"])
def test_vio_with_the_resident_prior(backend_cls, monkeypatch, form):
    """Kept landmarks and 15 x 15 blocks behind the resident dense prior; the pseudo-observations of its sparsified factors."""
    _env(monkeypatch, sqrt=1)
    w, args, w2, keep = ch.vio_marg_step()
    be = backend_cls(device=0)
    try:
        be.set_prior(ch.VIO_J0, np.zeros(15))
        be.set_windows([w])
        g = be.marginalize(0, form="cholesky", readback=True, **args)
        assert g is not None and g["n_full"] == g["n"]
        resident = {k: v for k, v in g.items() if k not in ("J", "r0")}
        resident["resident"] = True
        fs = be.sparsify(0, resident, vio=True) if form == "sparse" else None
        w_ref = ch.vio_attach(w, w2, keep, g, fs)
        w_dev = w_ref
        if form == "dense":
            w_dev = dataclasses.replace(w_ref, dense_prior=dict({k: v for k, v in w_ref.dense_prior.items() if k not in ("J", "r0")}, resident=True))
        be.set_windows([w_dev])
        be.solve(_opts())
        d = be.get_deltas(0)
        pairs = [(0, 3), (1, 2)]
        c = be.covariance(0, kf=list(range(4)), pairs=pairs, lmk="all")
    finally:
        be.close()
    assert c["kf"].shape == (4, 15, 15)
    _check_family("vio_" + form, w_dev, d, c, pairs=pairs, w_ref=w_ref)


def test_landmark_with_64_observations(backend_cls, monkeypatch):
    """The 128-row factorisation on one lane."""
    _env(monkeypatch, sqrt=1)
    w = ch.window_obs64()
    d, c, _ = _solve_cov(backend_cls, w, pairs=[(0, 30)])
    _check_family("obs64", w, d, c, pairs=[(0, 30)])


def test_600_landmark_window(backend_cls, monkeypatch):
    _env(monkeypatch, sqrt=1)
    w = ch.window_lmk600()
    d, c, _ = _solve_cov(backend_cls, w, want_kf=False)
    _check_family("lmk600", w, d, c, want_kf=False)


# ---- 4: bits -----------------------------------------------------------------------------------------------------------------------
def test_bits_under_sqrt_1(backend_cls, monkeypatch):
    _env(monkeypatch, sqrt=1)
    w = sh.window_near(1e-3, True)
    be = backend_cls(device=0)
    try:
        be.set_windows([w]); be.solve(_opts())
        d0 = be.get_deltas(0)
        c1 = be.covariance(0, kf=list(range(6)), pairs=PAIRS, lmk="all")
        d1 = be.get_deltas(0)
        c2 = be.covariance(0, kf=list(range(6)), pairs=PAIRS, lmk="all")
        c3 = be.covariance(0, kf=[4], pairs=[(0, 4)], lmk=[sh.NEAR_LMK, 5])
    finally:
        be.close()
    assert _same(c1, c2)
    assert all(d0[k].tobytes() == d1[k].tobytes() for k in d0)
    assert np.array_equal(c1["pair"][0], c1["pair"][1].T)
    assert c3["kf"][0].tobytes() == c1["kf"][4].tobytes() and c3["pair"][0].tobytes() == c1["pair"][2].tobytes()
    assert c3["lmk"][0].tobytes() == c1["lmk"][sh.NEAR_LMK].tobytes() and c3["lmk"][1].tobytes() == c1["lmk"][5].tobytes()
    dg, cg, _ = _solve_cov(backend_cls, w, pairs=PAIRS, use_graph=True)
    same = all(d0[k].tobytes() == dg[k].tobytes() for k in d0)
    print(f"[cov sqrt] graph against graph-less: deltas bit-identical {same}")
    _check_near("near_1e-3_noisy", w, dg, cg, tag=" (graph handle)")
    if same:
        assert _same(c1, cg)


# ---- 5: the band route -------------------------------------------------------------------------------------------------------------
def test_band_route_under_sqrt_1(backend_cls, monkeypatch):
    _env(monkeypatch, sqrt=1, band=1)
    w = cbh.window_vo12()
    pairs = [(0, 1), (3, 1), (0, 10), (10, 0)]
    d, c, times = _solve_cov(backend_cls, w, pairs=pairs, profile=True)
    assert "cov_band" in times and "cov_assemble_sqrt" in times and "cov_invert" not in times, sorted(times)
    info = ch.Information(w, d, 0.0)
    ref = ch.reference_blocks(info)
    got = {"kf": c["kf"], "pair": c["pair"], "lmk": c["lmk"]}
    want = {"kf": ref["kf"], "pair": [ref["cross"](a, b) for a, b in pairs], "lmk": ref["lmk"]}
    m = cbh.worst(got, want)
    tol = ch.TOL_FACTOR * cbh.E_REF["vo12"]
    print(f"[cov sqrt] band route, vo12: worst relative block difference {m:.3e}; bound {tol:.3e}")
    assert m <= tol
    assert np.array_equal(c["pair"][2], c["pair"][3].T)


def test_band_route_serves_a_near_landmark_through_the_retry(backend_cls, monkeypatch):
    _env(monkeypatch, band=1)
    w = sh.window_band_near(1e-4)
    pairs = [(0, 1), (0, 10), (10, 0)]                      # in the band | outside it, both orders
    d, c, times = _solve_cov(backend_cls, w, pairs=pairs, profile=True)
    assert c["rc"] == capi.SADVIO_OK
    assert "cov_band" in times and "cov_assemble_sqrt" in times and "cov_assemble" in times, sorted(times)
    _check_near("band_near_1e-4", w, d, c, pairs=pairs)
    assert np.array_equal(c["pair"][1], c["pair"][2].T)


# ---- 6: the unanchored window ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sqrt", [None, 1])
def test_unanchored_window_is_not_usable(backend_cls, monkeypatch, sqrt):
    _env(monkeypatch, sqrt=sqrt)
    w = synthetic.make_window(n_kf=4, n_lmk=60, obs_per_lmk=4, seed=33, fixed=0)
    w.pose_priors = []
    be = backend_cls(device=0)
    try:
        be.set_windows([w]); be.solve(_opts())
        r = be.covariance(0, kf=[0, 1], pairs=[(0, 1)], lmk="all", raw_rc=True)
    finally:
        be.close()
    assert r["rc"] == capi.E_NOT_USABLE and "positive definite" in r["error"]
    assert np.all(r["kf"] == 0.0) and np.all(r["pair"] == 0.0) and np.all(r["lmk"] == 0.0)


# ---- 7: batch ----------------------------------------------------------------------------------------------------------------------
def _batch(backend_cls, ws, items, frozen=False):
    be = backend_cls(device=0)
    try:
        be.set_windows(ws); be.solve(_opts(frozen=frozen))
        d = [be.get_deltas(k) for k in range(len(ws))]
        out = be.covariance_batch(items, fill=7.5)
    finally:
        be.close()
    return d, out


def test_batch(backend_cls, monkeypatch):
    """[near 0.1 mm, pixel_vo] in one call. Unset: the near item's unit fails the in-LDS pivot test and is retried on its own in
    square-root form, the pixel_vo item keeps the bits of SADVIO_COV_SQRT=0. 1: both down the DENSE route, both within their bars."""
    ws = [sh.window_near(1e-4), ch.window_pixel_vo()]
    items = [dict(w=0, kf=list(range(6)), pairs=PAIRS, lmk="all"), dict(w=1, kf=[0, 1, 2], pairs=[(0, 1), (1, 0)], lmk="all")]
    _env(monkeypatch)
    d, got = _batch(backend_cls, ws, items)
    assert [g["status"] for g in got] == [capi.SADVIO_OK, capi.SADVIO_OK]
    assert got[1]["route"] == capi.COV_ROUTE_LDS
    _check_near("near_1e-4", ws[0], d[0], got[0], tag=" (batch, unset)")
    _check_family("pixel_vo", ws[1], d[1], got[1], pairs=[(0, 1), (1, 0)])
    du, gotu = _batch(backend_cls, ws, items, frozen=True)          # bits: both handles frozen at the constructed state (_opts)
    _env(monkeypatch, sqrt=0)
    d0, got0 = _batch(backend_cls, ws, items, frozen=True)
    assert all(_zero(x) for x in du + d0)
    assert [g["status"] for g in gotu] == [capi.SADVIO_OK, capi.SADVIO_OK]
    assert got0[0]["status"] == capi.E_NOT_USABLE and got0[1]["status"] == capi.SADVIO_OK
    assert all(np.all(got0[0][k] == 7.5) for k in ("kf", "pair", "lmk"))
    assert _same(gotu[1], got0[1]) and gotu[1]["n_lmk_singular"] == got0[1]["n_lmk_singular"] == 1
    assert gotu[1]["route"] == got0[1]["route"] == capi.COV_ROUTE_LDS
    _env(monkeypatch, sqrt=1)
    d1, got1 = _batch(backend_cls, ws, items)
    assert [g["status"] for g in got1] == [capi.SADVIO_OK, capi.SADVIO_OK]
    assert [g["route"] for g in got1] == [capi.COV_ROUTE_DENSE, capi.COV_ROUTE_DENSE]
    _check_near("near_1e-4", ws[0], d1[0], got1[0], tag=" (batch, 1)")
    _check_family("pixel_vo", ws[1], d1[1], got1[1], pairs=[(0, 1), (1, 0)])


# ---- 8: window index ---------------------------------------------------------------------------------------------------------------
def test_near_window_behind_a_decoy(backend_cls, monkeypatch):
    """The near window at index 1 behind a decoy of tests/batch_helpers.py: the bits it has at index 0 of the same two-window batch."""
    _env(monkeypatch)
    w = sh.window_near(1e-4)
    req = dict(kf=list(range(6)), pairs=PAIRS, lmk="all")
    res = {}
    for at in (0, 1):
        ws = [w, bh.decoy(bh.PIXEL, "a")] if at == 0 else [bh.decoy(bh.PIXEL, "a"), w]
        be = backend_cls(device=0)
        try:
            be.set_windows(ws); be.solve(_opts(frozen=True))    # bits of two handles: both frozen at the constructed state (_opts)
            res[at] = (be.get_deltas(at), be.covariance(at, **req))
        finally:
            be.close()
    assert _zero(res[0][0]) and _zero(res[1][0])
    _check_near("near_1e-4", w, res[1][0], res[1][1], tag=" (window 1)")
    assert _same(res[0][1], res[1][1]) and res[0][1]["n_lmk_singular"] == res[1][1]["n_lmk_singular"] == 0
