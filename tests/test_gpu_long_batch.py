"""sadvio_ba_covariance_batch, sadvio_ba_marginalize_relative and sadvio_ba_marginalize_relative_batch on windows with long tracks
(landmarks of more than 64 observations), on handles created with SADVIO_CFG_LONG_TRACK_BATCH (capi.Backend(long_track_batch=True);
cov_batch_kernels.h: k_covb_long / k_covb_lmk_long, rel_runs.h).

Covariances: the reference and the bar are those of tests/test_gpu_long_cov.py (its _check: cov_helpers.reference_blocks of
cov_helpers.Information at the device's own deltas; a block passes at cov_helpers.TOL_FACTOR x long_cov_helpers.E_REF of its window).
Items that go through the single call's steps (DENSE, BAND, SADVIO_COV_SQRT=1) and NONE items carry the bits of sadvio_ba_covariance
on the same handle. Relative marginalisation: the oracle's single-pair routine under tests/test_gpu_relative_batch.py's check_pair,
and, to the bit, the same pair on a handle without flags on the window whose long tracks are cut to the pair's two key-frames: the
bisection must give what the walk gives. Every case prints its figures (LONGBATCH ...) before it asserts."""
import dataclasses

import numpy as np
import pytest

import batch_helpers as bt
import cov_helpers as ch
import long_cov_helpers as lc
import long_track_helpers as lh
from sadvio_amd import capi
from test_gpu_long_cov import _check
from test_gpu_relative_batch import AK_TOL, COND_MAX, INF_TOL, OK, REFUSED, T_a_b_of, check_pair, is_zero, shared_counts

pytestmark = pytest.mark.gpu

REL = dict(long_tracks=True, long_track_batch=True)                                  # 1 | 8
COV = dict(long_tracks=True, long_track_covariance=True, long_track_batch=True)      # 1 | 4 | 8
ALL = dict(COV, long_track_priors=True)                                              # 1 | 2 | 4 | 8
NONE, LDS, DENSE, BAND = capi.COV_ROUTE_NONE, capi.COV_ROUTE_LDS, capi.COV_ROUTE_DENSE, capi.COV_ROUTE_BAND
KEYS = ("kf", "pair", "lmk")
REL_KEYS = ("inf", "Ak", "T_a_b", "n_shared", "status")
NEW_CLASSES = ("k_covb_long", "k_covb_lmk_long")


def _env(monkeypatch, **kw):
    for key in ("SADVIO_COV_SQRT", "SADVIO_COV_BAND", "SADVIO_LONG_MIN", "SADVIO_COV_BATCH_LDS"):
        val = kw.get(key[len("SADVIO_"):].lower())
        if val is None:
            monkeypatch.delenv(key, raising=False)
        else:
            monkeypatch.setenv(key, str(val))


def _item(w, idx=0, pairs=None):
    return dict(w=idx, kf=list(range(w.n_kf)), pairs=[lc.far_pair(w)] if pairs is None else pairs, lmk="all")


def _same(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in KEYS) and a["n_lmk_singular"] == b["n_lmk_singular"]


def _state(be, idx=0):
    d = be.get_deltas(idx)
    pr = be.get_prior()
    return {**{f"delta {k}": v.tobytes() for k, v in d.items()}, "trace": be.get_trace(idx).tobytes(),
            "prior": (pr["valid"], pr["n_full"], pr["n"], pr.get("J", np.zeros(0)).tobytes(), pr.get("r0", np.zeros(0)).tobytes())}


# ---- 1. flags ---------------------------------------------------------------------------------------------------------------------------
def test_flags(backend_cls, monkeypatch):
    _env(monkeypatch)
    with pytest.raises(capi.SadvioError, match="SADVIO_CFG_LONG_TRACK_BATCH needs SADVIO_CFG_LONG_TRACKS"):
        backend_cls(device=0, long_track_batch=True)
    for flags in (REL, COV, ALL):
        backend_cls(device=0, **flags).close()
    w = lc.window("MIX")
    # 1 | 8: the batch covariance call keeps refusing, with the text; nothing of the solve is touched
    be = backend_cls(device=0, **REL)
    try:
        be.set_windows([w]); be.solve(lc.options("MIX"))
        s0 = _state(be)
        r = be.covariance_batch([dict(w=0, kf=[0], lmk="all")], raw_rc=True)
        assert r["rc"] == capi.E_INVALID_ARG and lh.LONG_TEXT in r["error"] and "covariance_batch" in r["error"]
        assert _state(be) == s0
        assert be.marginalize_relative_batch(0, [(0, 1)])["status"].shape == (1,)   # ... while the relative calls are served
    finally:
        be.close()
    # 1 | 2 | 4: all three still refuse
    be = backend_cls(device=0, long_tracks=True, long_track_priors=True, long_track_covariance=True)
    try:
        be.set_windows([w]); be.solve(lc.options("MIX"))
        r = be.covariance_batch([dict(w=0, kf=[0], lmk="all")], raw_rc=True)
        assert r["rc"] == capi.E_INVALID_ARG and lh.LONG_TEXT in r["error"] and "covariance_batch" in r["error"]
        with pytest.raises(capi.SadvioError, match=lh.LONG_TEXT):
            be.marginalize_relative(0, 0, 1)
        with pytest.raises(capi.SadvioError, match=lh.LONG_TEXT):
            be.marginalize_relative_batch(0, [(0, 1)])
    finally:
        be.close()


# ---- 2. the LDS route against the project's bar -------------------------------------------------------------------------------------
LDS_NP = {"L65": 30, "L65_angular": 30, "L65_huber": 30, "MIX": 36, "VIO": 90, "C128": 60, "C129": 60, "W300": 60}


def _lds_case(backend_cls, name, w, flags, label=""):
    pairs = [lc.far_pair(w)]
    be = backend_cls(device=0, profile_kernels=True, **flags)
    try:
        be.set_windows([w]); be.solve(lc.options(name))
        d = be.get_deltas(0)
        got = be.covariance_batch([_item(w)])[0]
        kt = be.kernel_times()
    finally:
        be.close()
    assert got["route"] == LDS and got["status"] == OK, (got["route"], got["status"])
    _check(name, w, d, got, pairs, label=f" [covariance_batch, LDS route{label}]")
    print(f"LONGBATCH {name}{label}: classes {sorted(k for k in kt if 'cov' in k)}")
    for cls in NEW_CLASSES:
        assert cls in kt, (cls, sorted(kt))
    return got


@pytest.mark.parametrize("name", list(LDS_NP))
def test_lds_route(backend_cls, monkeypatch, name):
    _env(monkeypatch)
    w = lc.window(name)
    assert len(lh.long_landmarks(w)) >= 1
    d_state = 15 if w.has_imu else 6
    assert d_state * len(lc.free_kfs(w)) == LDS_NP[name]
    _lds_case(backend_cls, name, w, COV)


def test_lds_route_kept_long_tracks(backend_cls, oracle_lib, monkeypatch):
    import long_prior_helpers as ph
    _env(monkeypatch)
    w = ph.case_prior_window(ph.CASE["KMIX"], oracle_lib)
    kept = sorted(set(int(l) for l, col in zip(w.dense_prior["lmk_index"], w.dense_prior["lmk_col"]) if col >= 0) & set(lh.long_landmarks(w).tolist()))
    assert len(kept) == 3
    got = _lds_case(backend_cls, "KMIX", w, ALL, label=", under its prior")
    for l in kept:   # COV_LMK_REDUCED: the block is read from Sigma_pp
        assert np.all(np.linalg.eigvalsh(got["lmk"][l]) > 0)


# ---- 3. routes that go through the single call's steps, and NONE -----------------------------------------------------------------------
def _mix_all_constant():
    w = lc.window("MIX")
    return dataclasses.replace(w, kf_const=np.ones(w.n_kf, dtype=np.asarray(w.kf_const).dtype))


@pytest.mark.parametrize("case", ["F70", "BIG", "BANDL", "MIX_sqrt", "MIX_none"])
def test_routes_with_the_single_calls_bits(backend_cls, monkeypatch, case):
    name = case.split("_")[0]
    _env(monkeypatch, cov_band=1 if case == "BANDL" else None, cov_sqrt=1 if case == "MIX_sqrt" else None)
    w = _mix_all_constant() if case == "MIX_none" else lc.window(name)
    want = {"F70": DENSE, "BIG": DENSE, "BANDL": BAND, "MIX_sqrt": DENSE, "MIX_none": NONE}[case]
    free = lc.free_kfs(w)
    pairs = [lc.far_pair(w)] if len(free) >= 2 else []
    be = backend_cls(device=0, profile_kernels=True, **COV)
    try:
        be.set_windows([w]); be.solve(lc.options(name))
        d = be.get_deltas(0)
        got = be.covariance_batch([_item(w, pairs=pairs)])[0]
        one = be.covariance(0, kf=list(range(w.n_kf)), pairs=pairs, lmk="all")
        kt = be.kernel_times()
    finally:
        be.close()
    print(f"LONGBATCH {case}: route {got['route']} (expected {want}), N_p {6 * len(free)}; classes {sorted(k for k in kt if 'cov' in k)}")
    assert got["route"] == want and got["status"] == OK
    assert _same(got, one), f"{case}: the batch item differs from sadvio_ba_covariance on the same handle"
    assert np.isfinite(got["lmk"]).all() and got["n_lmk_singular"] == 0
    if case == "MIX_none":   # the group path: the unit kernels ran, and gave the single call's bits
        assert all(cls in kt for cls in NEW_CLASSES) and np.all(got["kf"] == 0.0)
        assert np.all(got["lmk"][31] == 0.0) and np.all(np.linalg.eigvalsh(got["lmk"][0]) > 0)
    else:
        assert not any(cls in kt for cls in NEW_CLASSES)
        _check(name, w, d, got, pairs, label=f" [covariance_batch, {case}]")


# ---- 4. independence, determinism, window index ----------------------------------------------------------------------------------------
def test_independence_determinism_window_index(backend_cls, monkeypatch):
    _env(monkeypatch)
    ws = [bt.decoy(bt.PIXEL, "a"), lc.window("MIX"), lc.window("W300")]
    items = [_item(ws[1], 1), _item(ws[2], 2), _item(ws[0], 0, pairs=[(0, 1)]), dict(w=1, kf=[lc.free_kfs(ws[1])[0]], lmk=[62, 0, 5, 31])]
    be = backend_cls(device=0, profile_kernels=True, **COV)
    try:
        be.set_windows(ws); be.solve(capi.gn_options(4))
        d = {i: be.get_deltas(i) for i in (1, 2)}
        first = be.covariance_batch(items)
        again = be.covariance_batch(items)
        alone = [be.covariance_batch([it])[0] for it in items]
        n_long_launches = {c: be.kernel_times()[c]["launches"] for c in NEW_CLASSES}
        decoy_only = be.covariance_batch([items[2]])[0]
        after = {c: be.kernel_times()[c]["launches"] for c in NEW_CLASSES}
    finally:
        be.close()
    assert [g["route"] for g in first] == [LDS, LDS, LDS, LDS] and all(g["status"] == OK for g in first)
    for i, (a, b, c) in enumerate(zip(first, again, alone)):
        assert _same(a, b), f"item {i}: a second call differs"
        assert _same(a, c), f"item {i}: its bits depend on the other items of the call"
    assert _same(first[2], decoy_only) and after == n_long_launches   # a call that names no long window: the same bits, no new launch
    assert first[3]["lmk"][1].tobytes() == first[0]["lmk"][0].tobytes() and first[3]["lmk"][0].tobytes() == first[0]["lmk"][62].tobytes()
    assert first[3]["kf"][0].tobytes() == first[0]["kf"][lc.free_kfs(ws[1])[0]].tobytes()
    _check("MIX", ws[1], d[1], first[0], [lc.far_pair(ws[1])], label=" [window 1 of 3]")
    _check("W300", ws[2], d[2], first[1], [lc.far_pair(ws[2])], label=" [window 2 of 3]")
    print("LONGBATCH [decoy, MIX, W300]: two calls bit-identical; every item equals the item alone; the decoy's item equals a call without long windows")


# ---- 5. SADVIO_LONG_MIN=2: every landmark of at least 2 observations down the long path -------------------------------------------
def test_long_min_2(backend_cls, monkeypatch):
    _env(monkeypatch, long_min=2)
    w = lc.window("MIX")
    assert lh.counts(w).min() >= 2
    _lds_case(backend_cls, "MIX", w, COV, label=", SADVIO_LONG_MIN=2")


# ---- 6. the relative marginalisations against the oracle -------------------------------------------------------------------------------
def _best_pair(w, l):
    """The two key-frames long track l is seen from that share the most landmarks (ties: the first in index order)."""
    m = np.zeros((w.n_lmk, w.n_kf), dtype=np.int64)
    m[np.repeat(np.arange(w.n_lmk), np.diff(w.lmk_obs_ptr)), w.obs_kf] = 1
    k = np.flatnonzero(m[l])
    sh = (m.T @ m)[np.ix_(k, k)]
    np.fill_diagonal(sh, -1)
    i, j = np.unravel_index(np.argmax(sh), sh.shape)
    return int(k[min(i, j)]), int(k[max(i, j)])


def _rel_pairs(w, l):
    """Pairs around long track l: its first and last key-frame as a and as b, a > b, a key-frame in the middle of the track, its two
    one the track is not seen from (where there is one), and a duplicate.
    (Not among them: the track's two key-frames that share the MOST landmarks, _best_pair. There inf is at the mercy of the noise-floor
    cut on Ak, whatever finds the observations: an eigenvalue of Ak's gauge null space lies at the cut (L65_angular (1, 2): 1.86e-6 in the
    oracle against a cut of 1.99e-6), two summation orders keep or drop it, and inf is off by O(1) — measured 8.1e-01 for the single-pair
    call on L65_angular (1, 2) and 9.9e-01 for both calls on C129 (67, 68), with the same figures from the commit before this one on the
    window cut to 64 observations. Ak, which the bisection feeds, agrees to 1e-12 on all of them.)"""
    k = np.unique(w.obs_kf[w.lmk_obs_ptr[l]:w.lmk_obs_ptr[l + 1]])
    first, last, mid = int(k[0]), int(k[-1]), int(k[len(k) // 2])
    pairs = [(first, last), (last, first), (first, mid), (mid, last), (last, mid)]
    outside = [kf for kf in range(w.n_kf) if kf not in set(k.tolist())]
    if outside:
        pairs += [(outside[0], mid), (mid, outside[0])]
    return pairs + [pairs[0]]


def _check_pair(got, i, w, a, b, ref, fig):
    """check_pair; a pair whose oracle inf is not finite (the long track alone is shared: J Sigma_k J^T has rank 3 and the oracle's own
    inverse overflows, which check_pair's numpy.linalg.cond cannot take) is held on Ak, T_a_b and the zeros of a refusal, with
    check_pair's figures."""
    if ref is None or np.isfinite(ref[0]).all():
        return check_pair(got, i, w, a, b, ref, True, fig)
    st = int(got["status"][i])
    assert st in (OK, REFUSED)
    if st == REFUSED:
        assert is_zero(got, i)
        return False
    e_ak = np.abs(got["Ak"][i] - ref[1]).max() / np.abs(ref[1]).max()
    fig["Ak"] = max(fig.get("Ak", 0.0), e_ak)
    assert e_ak <= AK_TOL, f"pair ({a}, {b}): |Ak - ref| / max = {e_ak:.3e}"
    assert np.abs(got["T_a_b"][i] - T_a_b_of(w, a, b)).max() <= 1e-14
    return False


@pytest.mark.parametrize("name", ["MIX", "L65_angular", "C129", "W300"])
def test_relative_against_the_oracle(backend_cls, oracle_lib, monkeypatch, name):
    _env(monkeypatch)
    w = lc.window(name)
    l = int(lh.long_landmarks(w)[0])
    pairs = _rel_pairs(w, l)
    be = backend_cls(device=0, **REL)
    try:
        be.set_windows([w])
        got = be.marginalize_relative_batch(0, pairs)
        single = [be.marginalize_relative(0, a, b) for a, b in pairs[:-1]]
    finally:
        be.close()
    fig, fig1, n_inf = {}, {}, 0
    for i, (a, b) in enumerate(pairs):
        ref = oracle_lib.marginalize_relative(w, a, b)
        n_sh = shared_counts(w, a, b)[0]
        assert (ref is None) == (n_sh == 0)
        n_inf += _check_pair(got, i, w, a, b, ref, fig)
        if ref is not None and got["status"][i] == OK:
            assert got["n_shared"][i] == n_sh
        if i == len(pairs) - 1:
            for key in REL_KEYS:
                assert np.array_equal(got[key][i], got[key][0]), f"{key}: the duplicate pair differs from its first occurrence"
            continue
        one = single[i]   # the single-pair call, held as tests/test_gpu_relative_batch.py holds it
        if ref is None:
            assert one is None, (a, b)
        if one is None:   # refused: nothing shared, or a covariance the oracle too can barely invert (the batch refuses that pair as well)
            assert ref is None or (got["status"][i] == REFUSED and not (np.isfinite(ref[0]).all() and np.linalg.cond(ref[0]) <= COND_MAX)), (a, b)
            continue
        e_ak = np.abs(one[1] - ref[1]).max() / np.abs(ref[1]).max()
        fig1["Ak"] = max(fig1.get("Ak", 0.0), e_ak)
        assert e_ak <= AK_TOL, (a, b, e_ak)
        if np.isfinite(ref[0]).all() and np.linalg.cond(ref[0]) <= COND_MAX:
            e_inf = np.abs(one[0] - ref[0]).max() / np.abs(ref[0]).max()
            fig1["inf"] = max(fig1.get("inf", 0.0), e_inf)
            assert e_inf <= INF_TOL, (a, b, e_inf)
    shared_long = sum(1 for a, b in pairs if {a, b} <= set(w.obs_kf[w.lmk_obs_ptr[l]:w.lmk_obs_ptr[l + 1]].tolist()))
    print(f"LONGBATCH {name} relative: {len(pairs)} pairs around long track {l} ({lh.counts(w)[l]} observations; {shared_long} pairs share it), "
          f"inf compared on {n_inf}; batch worst {fig}; single-pair call worst {fig1}")
    assert shared_long >= 5


# ---- 7. bisection equals walk, to the bit -----------------------------------------------------------------------------------------------
def _cut_window(w, a, b):
    """w with the observations of every long track in key-frames other than a and b removed (at most 64 are left of each: a window a
    handle without flags takes). Only the long tracks change."""
    import test_gpu_tile_packing as tp
    picks = []
    for l in range(w.n_lmk):
        k = w.obs_kf[w.lmk_obs_ptr[l]:w.lmk_obs_ptr[l + 1]]
        picks.append((w, l, np.flatnonzero((k == a) | (k == b)) if len(k) > lh.MAX_TILE_OBS else None))
    cut = tp._assemble(w, picks)
    cut.lmk_const = None if w.lmk_const is None else np.asarray(w.lmk_const).copy()
    return cut


def test_bisection_equals_walk_to_the_bit(backend_cls, monkeypatch):
    _env(monkeypatch)
    w = lc.window("MIX")
    longs = lh.long_landmarks(w).tolist()
    a, b = _best_pair(w, 0)   # the two key-frames long track 0 is seen from that share the most landmarks
    cut = _cut_window(w, a, b)
    # on the host: the long tracks keep exactly their observations in a and b, nothing else changes
    assert cut.n_lmk == w.n_lmk and np.array_equal(cut.lmk_p, w.lmk_p) and np.array_equal(cut.kf_T_f_w, w.kf_T_f_w) and lh.counts(cut).max() <= lh.MAX_TILE_OBS
    for l in range(w.n_lmk):
        so, co = slice(w.lmk_obs_ptr[l], w.lmk_obs_ptr[l + 1]), slice(cut.lmk_obs_ptr[l], cut.lmk_obs_ptr[l + 1])
        keep = np.ones(so.stop - so.start, bool) if l not in longs else np.isin(w.obs_kf[so], (a, b))
        assert np.array_equal(cut.obs_kf[co], w.obs_kf[so][keep]) and np.array_equal(cut.obs_cam[co], w.obs_cam[so][keep]) and np.array_equal(cut.obs_meas[co], w.obs_meas[so][keep]), l
    assert 0 < (cut.lmk_obs_ptr[1] - cut.lmk_obs_ptr[0]) < lh.counts(w)[0]
    out = []
    for win, flags in ((w, REL), (cut, dict())):
        be = backend_cls(device=0, **flags)
        try:
            be.set_windows([win])
            out.append((be.marginalize_relative_batch(0, [(a, b), (b, a)]), be.marginalize_relative(0, a, b), be.marginalize_relative(0, b, a)))
        finally:
            be.close()
    (full_b, full_ab, full_ba), (cut_b, cut_ab, cut_ba) = out
    assert (full_b["status"] == OK).all() and full_b["n_shared"][0] == shared_counts(w, a, b)[0] == shared_counts(cut, a, b)[0] and full_b["Ak"].any()
    for key in REL_KEYS:
        assert full_b[key].tobytes() == cut_b[key].tobytes(), f"batch call, {key}: the bisection does not give the walk's bits"
    for (f, c), what in (((full_ab, cut_ab), "(a, b)"), ((full_ba, cut_ba), "(b, a)")):
        assert f is not None and c is not None
        assert f[0].tobytes() == c[0].tobytes() and f[1].tobytes() == c[1].tobytes(), f"single-pair call {what}: the bisection does not give the walk's bits"
    print(f"LONGBATCH MIX pair ({a}, {b}): {full_b['n_shared'][0]} shared landmarks; inf36, Ak144, T_a_b, n_shared and status of the full window (flags 1 | 8) "
          f"equal those of the cut window (no flags) byte for byte, batch call and single-pair call")


# ---- 8. the handle's state ---------------------------------------------------------------------------------------------------------------
def test_state_is_left_alone(backend_cls, monkeypatch):
    _env(monkeypatch)
    w = lc.window("MIX")
    be = backend_cls(device=0, **COV)
    try:
        be.set_windows([w]); be.solve(lc.options("MIX"))
        be.set_prior(np.eye(6)[:4], np.arange(4.0))
        s0 = _state(be)
        assert s0["prior"][0] is True
        be.covariance_batch([_item(w)])
        assert _state(be) == s0, "covariance_batch"
        be.marginalize_relative_batch(0, _rel_pairs(w, 0))
        assert _state(be) == s0, "marginalize_relative_batch"
        a, b = _rel_pairs(w, 0)[0]
        be.marginalize_relative(0, a, b)
        assert _state(be) == s0, "marginalize_relative"
    finally:
        be.close()
