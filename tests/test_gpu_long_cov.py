"""sadvio_ba_covariance and sadvio_ba_covariance_cross on windows with long tracks (landmarks of more than 64 observations), on handles
created with SADVIO_CFG_LONG_TRACKS | SADVIO_CFG_LONG_TRACK_COVARIANCE (sadvio_amd/csrc/cov_long_kernels.h).

The reference is cov_helpers.Information at the device's own deltas and the float64 inverse of the FULL information matrix
(reference_blocks): no 64-observation limit and no Schur complement on that side. A device block passes when
cov_helpers.worst_block_difference (every key-frame block, the nearest and the farthest pair of free key-frames, every landmark
block) is at most 64 x long_cov_helpers.E_REF of its window. Every case prints its figures (LONGCOV ...) before it asserts.

Two handles do not solve one window to the same bits (the solve's own sums are not ordered: tests/test_gpu_cov_band.py), so where a
case compares two handles it holds each to the bar at its own deltas and compares bits where the deltas came out bit-identical."""
import numpy as np
import pytest

import batch_helpers as bt
import cov_band_helpers as bh
import cov_cross_helpers as xh
import cov_helpers as ch
import long_cov_helpers as lc
import long_track_helpers as lh
from sadvio_amd import capi

pytestmark = pytest.mark.gpu

FLAGS = dict(long_tracks=True, long_track_covariance=True)


def _env(monkeypatch, sqrt=None, band=None):
    for key, val in (("SADVIO_COV_SQRT", sqrt), ("SADVIO_COV_BAND", band)):
        if val is None:
            monkeypatch.delenv(key, raising=False)
        else:
            monkeypatch.setenv(key, str(val))


def _pairs(w):
    return [lc.near_pair(w), lc.far_pair(w)]


def _solve_cov(backend_cls, name, w, pairs, flags=FLAGS, w_all=None, idx=0, **kw):
    """Solve (gn_options(4), the case's Huber a), then one covariance call for everything: (deltas, result, kernel classes)."""
    be = backend_cls(device=0, **flags, **kw)
    try:
        be.set_windows(w_all if w_all is not None else [w])
        be.solve(lc.options(name))
        d = be.get_deltas(idx)
        c = be.covariance(idx, kf=list(range(w.n_kf)), pairs=list(pairs), lmk="all")
        kt = be.kernel_times() if kw.get("profile_kernels") else {}
    finally:
        be.close()
    return d, c, kt


def _check(name, w, d, c, pairs, label="", w_ref=None):
    info = ch.Information(w_ref if w_ref is not None else w, d, lc.CASE[name].huber_a)
    ref = ch.reference_blocks(info)
    got = {"kf": c["kf"], "lmk": c["lmk"], "cross": lambda a, b: c["pair"][list(pairs).index((a, b))]}
    worst = ch.worst_block_difference(got, ref, info, pairs)
    bar = ch.TOL_FACTOR * lc.E_REF[name]
    longs = lh.long_landmarks(w)
    w_long = max(ch.rel_diff(c["lmk"][l], ref["lmk"][l]) for l in longs)
    print(f"LONGCOV {name}{label}: worst relative block difference {worst:.3e} (long tracks' blocks {w_long:.3e}); bar {bar:.3e} (64 x {lc.E_REF[name]:.1e})")
    assert np.isfinite(c["lmk"]).all() and c["n_lmk_singular"] == 0
    assert worst <= bar, (name, worst, bar)
    return info, ref


# ---- 1. every window, both assemblies, both routes -------------------------------------------------------------------------------
@pytest.mark.parametrize("sqrt", [0, 1])
@pytest.mark.parametrize("name", lc.TABLE)
def test_window(backend_cls, monkeypatch, name, sqrt):
    _env(monkeypatch, sqrt=sqrt)
    w = lc.window(name)
    assert len(lh.long_landmarks(w)) >= 1
    pairs = _pairs(w)
    d, c, kt = _solve_cov(backend_cls, name, w, pairs, profile_kernels=True)
    _check(name, w, d, c, pairs, label=f" [SADVIO_COV_SQRT={sqrt}]")
    assert "k_cov_long" in kt and "k_cov_lmk_long" in kt and ("cov_assemble_sqrt" if sqrt else "cov_assemble") in kt
    assert "cov_band" not in kt


@pytest.mark.parametrize("sqrt", [0, 1])
def test_band_route(backend_cls, monkeypatch, sqrt):
    """BANDL under SADVIO_COV_BAND=1: the long track's six free observers fill the band (hb = 5). Two neighbour pairs inside the band
    and one pair outside it."""
    _env(monkeypatch, sqrt=sqrt, band=1)
    w = lc.window("BANDL")
    f = lc.free_kfs(w)
    pairs = [(f[-1], f[-2]), (f[-3], f[-2]), (f[0], f[-1])]
    hb = bh.bandwidth(w)[0]
    fi = bh.free_index(w)
    assert [abs(int(fi[a] - fi[b])) <= hb for a, b in pairs] == [True, True, False]
    d, c, kt = _solve_cov(backend_cls, "BANDL", w, pairs, profile_kernels=True)
    _check("BANDL", w, d, c, pairs, label=f" [band route, SADVIO_COV_SQRT={sqrt}]")
    assert "cov_band" in kt and "cov_invert" not in kt and "k_cov_long" in kt and "k_cov_lmk_long" in kt


# ---- 2. constant long tracks ---------------------------------------------------------------------------------------------------------
def test_constant_long_tracks(backend_cls, monkeypatch):
    _env(monkeypatch)
    w = lc.window("MIX")
    pairs = _pairs(w)
    d, c, _ = _solve_cov(backend_cls, "MIX", w, pairs)
    _check("MIX", w, d, c, pairs)
    assert w.lmk_const[31] == 1 and np.all(c["lmk"][31] == 0.0) and c["n_lmk_singular"] == 0
    w2 = lc.with_const(w, 62)   # the last long track constant as well: its Jp^T Jp still counts, its W is zero
    d2, c2, _ = _solve_cov(backend_cls, "MIX", w2, pairs)
    _check("MIX", w2, d2, c2, pairs, label=" [last long track constant]")
    assert np.all(c2["lmk"][[31, 62]] == 0.0) and np.all(d2["lmk"][[31, 62]] == 0.0)
    assert ch.rel_diff(c2["kf"][0], c["kf"][0]) > ch.TOL_FACTOR * lc.E_REF["MIX"]   # the flag is really applied


# ---- 3. long tracks a prior keeps in the reduced system ----------------------------------------------------------------------------
@pytest.mark.parametrize("sqrt", [0, 1])
def test_kept_long_tracks(backend_cls, oracle_lib, monkeypatch, sqrt):
    import long_prior_helpers as ph
    _env(monkeypatch, sqrt=sqrt)
    w = ph.case_prior_window(ph.CASE["KMIX"], oracle_lib)
    kept = sorted(set(int(l) for l, col in zip(w.dense_prior["lmk_index"], w.dense_prior["lmk_col"]) if col >= 0) & set(lh.long_landmarks(w).tolist()))
    assert len(kept) == 3
    pairs = _pairs(w)
    d, c, _ = _solve_cov(backend_cls, "KMIX", w, pairs, flags=dict(FLAGS, long_track_priors=True))
    info, ref = _check("KMIX", w, d, c, pairs, label=f" [SADVIO_COV_SQRT={sqrt}]")
    bar = ch.TOL_FACTOR * lc.E_REF["KMIX"]
    for l in kept:   # COV_LMK_REDUCED: the block is read from Sigma_pp
        e = ch.rel_diff(c["lmk"][l], ref["lmk"][l])
        print(f"LONGCOV KMIX: kept long track {l}: {e:.3e}")
        assert e <= bar and np.all(np.linalg.eigvalsh(c["lmk"][l]) > 0)


# ---- 4. covariance_cross ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sqrt", [0, 1])
@pytest.mark.parametrize("name", lc.CROSS_WINDOWS)
def test_cross(backend_cls, monkeypatch, name, sqrt):
    """The newest free key-frame x every landmark, each with a candidate measurement."""
    _env(monkeypatch, sqrt=sqrt)
    w = lc.window(name)
    kf, lmk = lc.cross_candidates(w)
    be = backend_cls(device=0, **FLAGS)
    try:
        be.set_windows([w]); be.solve(lc.options(name))
        d = be.get_deltas(0)
        cam, meas = xh.candidate_observations(w, d, kf, lmk)
        got = be.covariance_cross(0, kf, lmk, cam, meas)
    finally:
        be.close()
    info = ch.Information(w, d, 0.0)
    X = np.linalg.inv(info.H)
    e_cross, e_innov = xh.worst_errors(w, info, X, d, kf, lmk, cam, meas, got)
    worst_block = max(ch.rel_diff(got["cross"][i], xh.cross_block(info, X, int(kf[i]), int(l))) for i, l in enumerate(lmk) if info.lmk_idx[l] is not None)
    t_cross, t_innov = ch.TOL_FACTOR * lc.E_REF[name], ch.TOL_FACTOR * lc.E_REF_INNOV.get(name, float('nan'))
    print(f"LONGCOV {name} cross [SADVIO_COV_SQRT={sqrt}]: {len(kf)} candidates, cross norm {e_cross:.3e}, worst block rel_diff {worst_block:.3e} "
          f"(bar {t_cross:.3e}), innovation {e_innov:.3e} (bar {t_innov:.3e})")
    assert e_cross <= t_cross and worst_block <= t_cross
    assert e_innov <= t_innov
    for l in lh.long_landmarks(w):
        i = int(np.flatnonzero(lmk == l)[0])
        assert got["status"][i] in (xh.CROSS_OK, xh.CROSS_PROJ_INVALID)
        assert np.all(got["cross"][i] == 0.0) == bool(w.lmk_const is not None and w.lmk_const[l])


# ---- 5. two calls, same bits ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sqrt", [0, 1])
@pytest.mark.parametrize("name", ["MIX", "W300"])
def test_two_calls_identical_and_solve_untouched(backend_cls, monkeypatch, name, sqrt):
    _env(monkeypatch, sqrt=sqrt)
    w = lc.window(name)
    pairs = _pairs(w)
    kf, lmk = lc.cross_candidates(w)
    be = backend_cls(device=0, **FLAGS)
    try:
        be.set_windows([w]); be.solve(lc.options(name))
        d0, t0 = be.get_deltas(0), be.get_trace(0)
        cam, meas = xh.candidate_observations(w, d0, kf, lmk)
        c1 = be.covariance(0, kf=list(range(w.n_kf)), pairs=pairs, lmk="all")
        x1 = be.covariance_cross(0, kf, lmk, cam, meas)
        c2 = be.covariance(0, kf=list(range(w.n_kf)), pairs=pairs, lmk="all")
        x2 = be.covariance_cross(0, kf, lmk, cam, meas)
        d1, t1 = be.get_deltas(0), be.get_trace(0)
    finally:
        be.close()
    for k in d0:
        assert d0[k].tobytes() == d1[k].tobytes(), k
    assert t0.tobytes() == t1.tobytes()
    for k in ("kf", "pair", "lmk"):
        assert c1[k].tobytes() == c2[k].tobytes(), k
    for k in ("cross", "innov", "maha2", "status"):
        assert x1[k].tobytes() == x2[k].tobytes(), k
    assert c1["n_lmk_singular"] == c2["n_lmk_singular"] == 0
    print(f"LONGCOV {name} [SADVIO_COV_SQRT={sqrt}]: two covariance and two covariance_cross calls bit-identical; deltas and trace untouched")


# ---- 6. graph handle -------------------------------------------------------------------------------------------------------------------------
def test_graph_handle(backend_cls, monkeypatch):
    _env(monkeypatch)
    w = lc.window("MIX")
    pairs = _pairs(w)
    d0, c0, _ = _solve_cov(backend_cls, "MIX", w, pairs)
    d1, c1, _ = _solve_cov(backend_cls, "MIX", w, pairs, use_graph=True)
    _check("MIX", w, d0, c0, pairs)
    _check("MIX", w, d1, c1, pairs, label=" [use_graph]")
    same = all(d0[k].tobytes() == d1[k].tobytes() for k in d0)
    print(f"LONGCOV MIX: graph against graph-less: deltas bit-identical {same}")
    if same:
        assert all(c0[k].tobytes() == c1[k].tobytes() for k in ("kf", "pair", "lmk"))


# ---- 7. nothing changes without long tracks ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["pixel_vo", "obs64"])
def test_windows_without_long_tracks_are_served_as_before(backend_cls, monkeypatch, case):
    """The same launches (no class of the long kernels) on a flags 1 | 4 handle as on a flags 0 handle, each within the window's own
    bar (cov_helpers.E_REF), and the same bits where the two solves returned the same bits."""
    _env(monkeypatch)
    w = {"pixel_vo": ch.window_pixel_vo, "obs64": ch.window_obs64}[case]()
    pairs = [(0, 1)]
    out = []
    for flags in (dict(), FLAGS):
        be = backend_cls(device=0, profile_kernels=True, **flags)
        try:
            be.set_windows([w]); be.solve(capi.reference_options())
            d = be.get_deltas(0)
            c = be.covariance(0, kf=list(range(w.n_kf)), pairs=pairs, lmk="all")
            kt = be.kernel_times()
        finally:
            be.close()
        info = ch.Information(w, d, 0.0)
        got = {"kf": c["kf"], "lmk": c["lmk"], "cross": lambda a, b: c["pair"][0]}
        worst = ch.worst_block_difference(got, ch.reference_blocks(info), info, pairs)
        print(f"LONGCOV {case} flags {sorted(flags)}: worst {worst:.3e}, bar {ch.TOL_FACTOR * ch.E_REF[case]:.3e}; classes {sorted(k for k in kt if 'cov' in k)}")
        assert worst <= ch.TOL_FACTOR * ch.E_REF[case]
        assert "k_cov_long" not in kt and "k_cov_lmk_long" not in kt and "k_cov_schur" not in kt and "k_cov_lmk" in kt
        out.append((d, c, sorted(k for k in kt if "cov" in k)))
    assert out[0][2] == out[1][2]
    same = all(out[0][0][k].tobytes() == out[1][0][k].tobytes() for k in out[0][0])
    print(f"LONGCOV {case}: deltas of the two handles bit-identical {same}")
    if same:
        for k in ("kf", "pair", "lmk"):
            assert np.array_equal(out[0][1][k], out[1][1][k], equal_nan=True) and np.array_equal(np.isnan(out[0][1][k]), np.isnan(out[1][1][k])), k


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals(backend_cls, monkeypatch):
    _env(monkeypatch)
    w = lc.window("MIX")
    be = backend_cls(device=0, **FLAGS)
    try:
        be.set_windows([w]); be.solve(lc.options("MIX"))
        d0, t0 = be.get_deltas(0), be.get_trace(0)
        r = be.covariance_batch([dict(w=0, kf=[0], lmk="all")], raw_rc=True)
        assert r["rc"] == capi.E_INVALID_ARG and lh.LONG_TEXT in r["error"] and "covariance_batch" in r["error"]
        with pytest.raises(capi.SadvioError, match=lh.LONG_TEXT):
            be.marginalize_relative(0, 0, 1)
        with pytest.raises(capi.SadvioError, match=lh.LONG_TEXT):
            be.marginalize_relative_batch(0, [(0, 1)])
        d1, t1 = be.get_deltas(0), be.get_trace(0)
        c = be.covariance(0, kf=[0], lmk=[0])   # and the handle still answers
    finally:
        be.close()
    for k in d0:
        assert d0[k].tobytes() == d1[k].tobytes(), k
    assert t0.tobytes() == t1.tobytes() and np.isfinite(c["lmk"]).all()
    with pytest.raises(capi.SadvioError, match="SADVIO_CFG_LONG_TRACK_COVARIANCE needs SADVIO_CFG_LONG_TRACKS"):
        backend_cls(device=0, long_track_covariance=True)
    for flags in (dict(long_tracks=True, long_track_covariance=True), dict(long_tracks=True, long_track_priors=True, long_track_covariance=True)):
        backend_cls(device=0, **flags).close()


# ---- 9. window index ---------------------------------------------------------------------------------------------------------------------------
def test_window_2_of_a_batch_behind_decoys(backend_cls, monkeypatch):
    _env(monkeypatch)
    w = lc.window("MIX")
    pairs = _pairs(w)
    d0, c0, _ = _solve_cov(backend_cls, "MIX", w, pairs)
    d2, c2, _ = _solve_cov(backend_cls, "MIX", w, pairs, w_all=[bt.decoy(bt.PIXEL, "a"), bt.decoy(bt.PIXEL, "b"), w], idx=2)
    _check("MIX", w, d0, c0, pairs)
    _check("MIX", w, d2, c2, pairs, label=" [window 2 of 3]")
    same = all(d0[k].tobytes() == d2[k].tobytes() for k in d0)
    print(f"LONGCOV MIX: window 2 behind decoys: deltas bit-identical to the window alone: {same}")
    if same:
        assert all(c0[k].tobytes() == c2[k].tobytes() for k in ("kf", "pair", "lmk"))
