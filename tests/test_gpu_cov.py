"""sadvio_ba_covariance on the device against the float64 inverse of the FULL information matrix (tests/cov_helpers.py: no Schur
complement on the reference side, so the elimination algebra is checked too), evaluated at the deltas the device's own solve
returned. A device block passes when its relative difference (max |got - ref| / max |ref|) from the helper's block is at most
TOL_FACTOR = 64 x E_REF of that window — E_REF is what float64 itself loses on that matrix against a 50-digit inverse
(tests/test_cov_cpu.py); the factor allows for the device's different summation order and the amplification of a few ulps of the
Jacobians by the conditioning of S. Every test prints its worst figure before it asserts.
"""
import dataclasses

import numpy as np
import pytest

import cov_helpers as ch
from sadvio_amd import capi, synthetic

pytestmark = pytest.mark.gpu


def _opts(huber=0.0):
    o = capi.reference_options()
    o.huber_a = huber
    return o


def _solve_cov(backend_cls, w, opts, pairs=(), use_graph=False, want_kf=True):
    be = backend_cls(device=0, use_graph=use_graph)
    try:
        be.set_windows([w])
        be.solve(opts)
        d = be.get_deltas(0)
        c = be.covariance(0, kf=list(range(w.n_kf)) if want_kf else None, pairs=list(pairs), lmk="all")
    finally:
        be.close()
    return d, c


def _check(case, w, d, c, huber=0.0, pairs=(), want_kf=True, w_ref=None):
    """Every key-frame block, the given cross pairs and every landmark block of c against the helper at the deltas d."""
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
    print(f"[cov] {case}: worst relative block difference kf {worst['kf']:.3e} pair {worst['pair']:.3e} lmk {worst['lmk']:.3e}; "
          f"bound {tol:.3e} (64 x e_ref {ch.E_REF[case]:.1e})")
    assert c["n_lmk_singular"] == len(info.singular)
    assert max(worst.values()) <= tol, (case, worst, tol)
    return info, ref


def test_pixel_vo_np_12(backend_cls):
    """Case 1: two free key-frames, all blocks and the cross pair; the single-observation landmark is NaN and counted."""
    w = ch.window_pixel_vo()
    d, c = _solve_cov(backend_cls, w, _opts(), pairs=[(0, 1), (1, 0)])
    info, _ = _check("pixel_vo", w, d, c, pairs=[(0, 1), (1, 0)])
    assert info.singular == [ch.SINGLE] and c["n_lmk_singular"] == 1
    assert np.isnan(c["lmk"][ch.SINGLE]).all()
    assert np.all(c["kf"][2] == 0.0)                                  # the constant key-frame
    assert np.array_equal(c["pair"][0], c["pair"][1].T)               # Sigma(a, b) = Sigma(b, a)^T
    for k in range(2):
        assert np.array_equal(c["kf"][k], c["kf"][k].T) and np.all(np.linalg.eigvalsh(c["kf"][k]) > 0)


def test_angular_vo_across_the_16_column_tile(backend_cls):
    """Case 2: angular factor, three free key-frames, N_p = 18."""
    w = ch.window_angular_vo()
    pairs = [(0, 1), (0, 2), (1, 2)]
    d, c = _solve_cov(backend_cls, w, _opts(), pairs=pairs)
    _check("angular_vo", w, d, c, pairs=pairs)


@pytest.mark.parametrize("form", ["dense", "sparse"])
def test_vio_with_the_resident_prior(backend_cls, form):
    """Case 3: 4 KF with IMU states and three IMU pairs behind a marginalisation that keeps 5 landmarks: the dense prior left
    resident on the handle, then its sparsified factors. 15 x 15 blocks; the prior-kept landmarks' blocks come from Sigma_pp."""
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
        w_ref = ch.vio_attach(w, w2, keep, g, fs)                     # what the helper reads: J, r0 on the host
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
    _check("vio_" + form, w_dev, d, c, pairs=pairs, w_ref=w_ref)
    kept = [int(np.flatnonzero(w_ref.lmk_id == w.lmk_id[l])[0]) for l in keep if len(np.flatnonzero(w_ref.lmk_id == w.lmk_id[l]))]
    assert len(kept) >= 1 and all(np.isfinite(c["lmk"][l]).all() and np.all(np.linalg.eigvalsh(c["lmk"][l]) > 0) for l in kept)


def test_huber(backend_cls):
    """Case 4: case 1 with three gross outliers under HuberLoss(sqrt(1.345)); the helper applies the same corrector."""
    w = ch.window_huber()
    d, c = _solve_cov(backend_cls, w, _opts(ch.HUBER_A), pairs=[(0, 1)])
    _check("huber", w, d, c, huber=ch.HUBER_A, pairs=[(0, 1)])
    _, c0 = _solve_cov(backend_cls, w, _opts(), pairs=[(0, 1)])
    assert ch.rel_diff(c["kf"][0], c0["kf"][0]) > 1e-3              # the corrector is really applied


def test_landmark_with_64_observations(backend_cls):
    """Case 5: 31 free key-frames; one landmark gathers 31 x 31 blocks of Sigma_pp."""
    w = ch.window_obs64()
    assert int(np.diff(w.lmk_obs_ptr)[ch.OBS64_LMK]) == 64
    d, c = _solve_cov(backend_cls, w, _opts(), pairs=[(0, 30)])
    _check("obs64", w, d, c, pairs=[(0, 30)])


def test_600_landmark_window(backend_cls):
    """Case 6: several landmark tiles and set-aside outlier tracks; landmark blocks only."""
    w = ch.window_lmk600()
    d, c = _solve_cov(backend_cls, w, _opts(), want_kf=False)
    assert c["kf"].shape[0] == 0
    _check("lmk600", w, d, c, want_kf=False)


# ---- contract ---------------------------------------------------------------------------------------------------------------------
def test_refusals(backend_cls, monkeypatch):
    from line_helpers import add_lines
    from sadvio_amd import sharding
    w = ch.window_angular_vo()
    be = backend_cls(device=0)
    try:
        be.set_windows([w])
        r = be.covariance(0, kf=[0], raw_rc=True)
        assert r["rc"] == capi.E_STATE and "before solve" in r["error"]
        be.solve(_opts())
        for kw in (dict(kf=[4]), dict(kf=[-1]), dict(pairs=[(0, 9)]), dict(lmk=[w.n_lmk]), dict(lmk=[-2])):
            r = be.covariance(0, raw_rc=True, **kw)
            assert r["rc"] == capi.E_INVALID_ARG and "out of range" in r["error"], kw
        assert be.covariance(1, kf=[0], raw_rc=True)["rc"] == capi.E_INVALID_ARG
        be._check(be.lib.sadvio_ba_begin_update(be.h), "begin_update")
        r = be.covariance(0, kf=[0], raw_rc=True)
        be._check(be.lib.sadvio_ba_commit_update(be.h), "commit_update")
        assert r["rc"] == capi.E_STATE and "begin_update" in r["error"]
    finally:
        be.close()
    # line landmarks
    wl = add_lines(synthetic.make_window(n_kf=4, n_lmk=60, obs_per_lmk=4, seed=21), n_line=3, obs_per_line=4)
    be = backend_cls(device=0)
    try:
        be.set_windows([wl]); be.solve(_opts())
        r = be.covariance(0, kf=[0], raw_rc=True)
        assert r["rc"] == capi.E_INVALID_ARG and "line landmarks" in r["error"]
    finally:
        be.close()
    # a window sharded over several GPUs
    be = backend_cls(device=0)
    try:
        be.set_collective(0, 2, lambda *a: 0)
        be.set_windows([sharding.shard_window(synthetic.make_window(n_kf=5, n_lmk=300, seed=42), 0, 2)])
        r = be.covariance(0, kf=[0], raw_rc=True)
        assert r["rc"] == capi.E_INVALID_ARG and "sharded" in r["error"]
    finally:
        be.close()
    # a batch the throughput kernels solved
    monkeypatch.setenv("SADVIO_LM", "1")
    be = backend_cls(device=0)
    try:
        be.set_windows([synthetic.make_window(n_kf=6, n_lmk=400, seed=7)]); be.solve(_opts())
        r = be.covariance(0, kf=[0], raw_rc=True)
        assert r["rc"] == capi.E_INVALID_ARG and "throughput" in r["error"]
    finally:
        be.close()


def test_unanchored_window_is_not_usable(backend_cls):
    """No constant key-frame, no prior: the gauge is free, S is singular. A return code, not a fault; outputs untouched."""
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


def test_constant_blocks_are_zero(backend_cls):
    w = ch.window_angular_vo()
    w.lmk_const = np.zeros(w.n_lmk, dtype=np.uint8)
    w.lmk_const[[3, 17]] = 1
    d, c = _solve_cov(backend_cls, w, _opts(), pairs=[(0, 3), (3, 3)])
    assert np.all(c["kf"][3] == 0.0) and np.all(c["pair"] == 0.0)
    assert np.all(c["lmk"][[3, 17]] == 0.0) and np.all(d["lmk"][[3, 17]] == 0.0)
    _check("angular_vo", w, d, c)


def test_solve_results_untouched_and_two_calls_identical(backend_cls):
    w = ch.window_pixel_vo()
    be = backend_cls(device=0)
    try:
        be.set_windows([w])
        s0 = be.solve(_opts())[0].as_dict()
        d0, t0 = be.get_deltas(0), be.get_trace(0)
        c1 = be.covariance(0, kf=[0, 1, 2], pairs=[(0, 1)], lmk="all")
        d1, t1 = be.get_deltas(0), be.get_trace(0)
        c2 = be.covariance(0, kf=[0, 1, 2], pairs=[(0, 1)], lmk="all")
        c3 = be.covariance(0, lmk=[5, ch.SINGLE, 5])                 # a selection, with a repeat; no key-frame output at all
    finally:
        be.close()
    for k in d0:
        assert d0[k].tobytes() == d1[k].tobytes(), k
    assert t0.tobytes() == t1.tobytes()
    assert s0["iterations"] == t0.shape[0] - 1
    for k in ("kf", "pair", "lmk"):
        assert c1[k].tobytes() == c2[k].tobytes(), k
    assert c3["lmk"][0].tobytes() == c1["lmk"][5].tobytes() == c3["lmk"][2].tobytes()
    assert np.isnan(c3["lmk"][1]).all() and c3["n_lmk_singular"] == 1 and c1["n_lmk_singular"] == 1


def test_graph_handle_gives_the_same_covariances(backend_cls):
    """use_graph = 1 only changes how the solve is launched. Where the two solves return the same bits, so must the two
    covariance calls; each is checked against the reference at its own deltas either way."""
    w = ch.window_angular_vo()
    pairs = [(0, 2)]
    d0, c0 = _solve_cov(backend_cls, w, _opts(), pairs=pairs)
    d1, c1 = _solve_cov(backend_cls, w, _opts(), pairs=pairs, use_graph=True)
    _check("angular_vo", w, d0, c0, pairs=pairs)
    _check("angular_vo", w, d1, c1, pairs=pairs)
    same = all(d0[k].tobytes() == d1[k].tobytes() for k in d0)
    worst = max([ch.rel_diff(c1["kf"][k], c0["kf"][k]) for k in range(w.n_kf)] + [ch.rel_diff(c1["lmk"][l], c0["lmk"][l]) for l in range(w.n_lmk)])
    print(f"[cov] graph against graph-less: deltas bit-identical {same}, worst relative block difference {worst:.3e}")
    if same:
        assert all(c0[k].tobytes() == c1[k].tobytes() for k in ("kf", "pair", "lmk"))
