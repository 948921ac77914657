"""Every per-window entry point of the C ABI called at a window index other than 0.

A handle concatenates the windows of a batch into global arrays and every auxiliary entry point does its own base arithmetic
(kf_base / cam_base / lmk_base / obs_base) on the host and in its kernels. Here the window under test always sits behind one or two
DECOYS (tests/batch_helpers.py: other sizes, other data, three cameras) so that a forgotten base reads wrong data, never equal
data; tests/test_window_index_cpu.py proves on the host that each decoy used here moves the target's linearisation by >= 1e-7
relative for each of the four bases. The targets are the windows of the single-window tests, the references are the oracle's
results for the target ALONE, and every bar is the one the single-window test of that entry point already holds (named where it is
used). Every test prints its worst figure before it asserts."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import batch_helpers as bh
import cov_helpers as ch
from sadvio_amd import capi
from test_gpu_cov import _check as cov_check
from test_gpu_marg import check_prior                      # rtol 1e-8 on J^T J and J^T r0
from test_gpu_relative_batch import AK_TOL, COND_MAX, INF_TOL, OK, REFUSED, check_pair, is_zero, raw_call, shared_counts
from test_gpu_sparsify import same_factors                 # rtol 1e-7 on the information square roots

pytestmark = pytest.mark.gpu
PIXEL, ANGULAR = capi.FACTOR_PIXEL, capi.FACTOR_ANGULAR
FACTORS = [PIXEL, ANGULAR]
LIN_TOL = 1e-10                      # tests/test_gpu_parity.py::test_linearize_matches_oracle
CHI2_TOL, CHI2_THRESHOLD_BAND = 1e-9, 1e-6   # tests/test_gpu_frontend.py::test_landmark_chi2_gate
REL_KEYS = ("inf", "Ak", "T_a_b", "n_shared", "status")
_ip = C.POINTER(C.c_int32)
_dp = C.POINTER(C.c_double)


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


# ---- linearize ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", FACTORS)
def test_linearize(backend_cls, oracle_lib, factor):
    """Every window of four batches (targets AND decoys) at zero and at random deltas, against the oracle on that window alone.
    The targets with an empty last / first landmark sit at the two ends of the probe's landmark search at a non-zero lmk_base."""
    a, b = bh.decoy(factor, "a"), bh.decoy(factor, "b")
    plain, last, first = bh.lin_target(factor), bh.lin_target(factor, "last"), bh.lin_target(factor, "first")
    assert last.lmk_obs_ptr[-1] == last.lmk_obs_ptr[-2] and first.lmk_obs_ptr[1] == 0 and last.n_obs == first.n_obs == plain.n_obs - 5
    batches = [[a, plain], [a, b, last], [b, first, a], [plain, a, b]]
    ref, figs = {}, []
    be = backend_cls(device=0)
    try:
        for ws in batches:
            be.set_windows(ws)
            for k in list(range(len(ws))) + [len(ws) - 1, 0]:        # ... and again out of order: a call leaves nothing behind
                w = ws[k]
                rng = np.random.default_rng(100 + w.n_obs)
                for pd, ld in [(None, None), (0.02 * rng.standard_normal((w.n_kf, 6)), 0.05 * rng.standard_normal((w.n_lmk, 3)))]:
                    key = (id(w), pd is None)
                    if key not in ref:
                        ref[key] = oracle_lib.linearize(w, pd, ld)[:3]
                    got = be.linearize(k, pd, ld)
                    figs.append((max(relerr(g, o) for g, o in zip(got, ref[key])), len(ws), k, pd is None))
    finally:
        be.close()
    print(f"[window index] linearize factor {factor}: worst relative difference {max(figs)[0]:.3e} (batch size, window, zero deltas: {max(figs)[1:]}); bar {LIN_TOL:.0e}")
    assert max(figs)[0] <= LIN_TOL, max(figs)


# ---- landmark_chi2 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", FACTORS)
def test_landmark_chi2(backend_cls, oracle_lib, factor):
    a, b, t = bh.decoy(factor, "a"), bh.decoy(factor, "b"), bh.chi2_target(factor)
    wh = np.tile([700.0, 460.0], (t.n_cam, 1))
    cmp, rest = [], []
    be = backend_cls(device=0)
    try:
        for ws, k in (([a, b, t], 2), ([t, a], 0)):
            be.set_windows(ws)
            be.solve(capi.landmark_optimization_options())
            before = [be.get_deltas(i) for i in range(len(ws))]
            d = before[k]
            calls = [{}, {"lmk_delta": d["lmk"]}, {"lmk_delta": d["lmk"], "image_wh": wh}]
            got = [be.landmark_chi2(k, **kw) for kw in calls]
            dec = [(i, be.landmark_chi2(i)) for i in range(len(ws)) if i != k]      # the decoys: three cameras, three sigmas
            after = [be.get_deltas(i) for i in range(len(ws))]
            cmp += [(av, fl) + oracle_lib.landmark_chi2(t, **kw) for (av, fl), kw in zip(got, calls)]
            cmp += [(av, fl) + oracle_lib.landmark_chi2(ws[i]) for i, (av, fl) in dec]
            rest.append((got, before, after))
    finally:
        be.close()
    worst = max((np.abs(av - ar) / (1.0 + np.abs(ar))).max() for av, fl, ar, fr in cmp)
    print(f"[window index] landmark_chi2 factor {factor}: worst |avg - oracle| / (1 + |oracle|) {worst:.3e}; bar rtol = atol = {CHI2_TOL:.0e}")
    for av, fl, ar, fr in cmp:
        assert np.allclose(av, ar, rtol=CHI2_TOL, atol=CHI2_TOL)
        sure = np.abs(ar - 2.0) > CHI2_THRESHOLD_BAND          # away from the threshold the flags are identical
        assert (fl[sure] == fr[sure]).all()
    for got, before, after in rest:
        (a0, i0), (a1, i1), (a2, i2) = got
        assert a0[3] == 1000.0 and i0[3] == 0 and i0[7] == 0
        assert i1.sum() > i0.sum() and i2.sum() <= i1.sum()
        for x, y in zip(before, after):              # the probe leaves the solved state of EVERY window readable
            for key in x:
                assert np.array_equal(x[key], y[key]), key


# ---- marginalize_relative / marginalize_relative_batch -----------------------------------------------------------------------------
def all_pairs(n):
    return [(i, j) for i in range(n) for j in range(n) if i != j]


_rel_refs = {}


def rel_refs(oracle_lib, w, tag, mode="noise_floor"):
    """The oracle's (inf, Ak, m) or None for every ordered pair of w, computed once."""
    key = (tag, w.factor_type, mode)
    if key not in _rel_refs:
        _rel_refs[key] = [oracle_lib.marginalize_relative(w, i, j, eig_cut=mode) for i, j in all_pairs(w.n_kf)]
    return _rel_refs[key]


def check_batch(got, w, refs, fig, compare_inf=True):
    """check_pair's rules (tests/test_gpu_relative_batch.py: Ak 1e-9, inf 1e-7 where the oracle's cond <= 1e7, zeros when refused)
    on every ordered pair; returns how many inf were compared."""
    n_inf = 0
    for i, (p, q) in enumerate(all_pairs(w.n_kf)):
        n_inf += check_pair(got, i, w, p, q, refs[i], compare_inf, fig)
        if refs[i] is not None and got["status"][i] == OK:
            assert got["n_shared"][i] == shared_counts(w, p, q)[0]
    return n_inf


@pytest.mark.parametrize("factor", FACTORS)
def test_marginalize_relative_in_slot_2(backend_cls, oracle_lib, factor):
    a, b, t = bh.decoy(factor, "a"), bh.decoy(factor, "b"), bh.rel_target(factor)
    pairs = all_pairs(t.n_kf)
    refs, refs0 = rel_refs(oracle_lib, t, "target"), rel_refs(oracle_lib, t, "target", "reference")
    be = backend_cls(device=0)
    try:
        be.set_windows([a, b, t])
        got = be.marginalize_relative_batch(2, pairs)
        got0 = be.marginalize_relative_batch(2, pairs, eig_cut="reference")
        single = [be.marginalize_relative(2, p, q) for p, q in pairs]
        be.set_windows([t, a])                              # something stored behind must not disturb it
        front = be.marginalize_relative_batch(0, pairs)
    finally:
        be.close()
    be = backend_cls(device=0)
    try:
        be.set_windows([t])
        alone = be.marginalize_relative_batch(0, pairs)
    finally:
        be.close()
    fig, fig1, n_inf = {}, {}, -1
    for (p, q), one, ref in zip(pairs, single, refs):       # the single-pair entry point: tests/test_gpu_relative.py's bars (the same two)
        if ref is not None and one is not None:
            fig1["Ak"] = max(fig1.get("Ak", 0.0), relerr(one[1], ref[1]))
            if np.linalg.cond(ref[0]) <= COND_MAX:
                fig1["inf"] = max(fig1.get("inf", 0.0), relerr(one[0], ref[0]))
    try:
        n_inf = check_batch(got, t, refs, fig)
        check_batch(got0, t, refs0, fig, compare_inf=False)
        check_batch(front, t, refs, fig)
    finally:
        print(f"[window index] relative factor {factor}: batch worst {fig}, inf compared on {n_inf}; single-pair call worst {fig1}")
    for (p, q), one, ref in zip(pairs, single, refs):
        if ref is None:
            assert one is None, (p, q)
            continue
        well = np.linalg.cond(ref[0]) <= COND_MAX
        assert one is not None or not well, (p, q)
    assert fig1["Ak"] <= AK_TOL and fig1["inf"] <= INF_TOL, fig1
    for p in ((0, 4), (4, 0)):                              # the two pairs that share nothing
        i = pairs.index(p)
        assert refs[i] is None and got["status"][i] == REFUSED and is_zero(got, i) and single[i] is None
    assert sum(r is not None for r in refs) == 18 and 18 - n_inf <= 2
    # rel_kernels.h: a pair's bits depend on (the window, a, b) alone — not on what else the handle holds, nor on the window's index
    same = {k: got[k].tobytes() == alone[k].tobytes() and front[k].tobytes() == alone[k].tobytes() for k in REL_KEYS}
    print(f"[window index] relative factor {factor}: slot 2 / slot 0 with a decoy behind bit-identical to the window alone: {same}")
    assert all(same.values()), same


@pytest.mark.parametrize("factor", FACTORS)
def test_relative_batch_landmark_lists_follow_the_window(backend_cls, oracle_lib, factor):
    """rel_index caches the per-key-frame landmark lists under the window index (RelScratch::csr_win): window 1, window 2, window 1
    again on one handle; then a second set_windows that puts another window at index 1."""
    a, b, t, o = bh.decoy(factor, "a"), bh.decoy(factor, "b"), bh.rel_target(factor), bh.rel_other(factor)
    be = backend_cls(device=0)
    try:
        be.set_windows([a, t, o])
        r1 = be.marginalize_relative_batch(1, all_pairs(t.n_kf))
        r2 = be.marginalize_relative_batch(2, all_pairs(o.n_kf))
        r3 = be.marginalize_relative_batch(1, all_pairs(t.n_kf))
        be.set_windows([b, o])
        r4 = be.marginalize_relative_batch(1, all_pairs(o.n_kf))
    finally:
        be.close()
    fig = {}
    refs_t, refs_o = rel_refs(oracle_lib, t, "target"), rel_refs(oracle_lib, o, "other")
    assert sum(r is not None for r in refs_o) >= 6
    n = []
    try:
        for r, w, refs in ((r1, t, refs_t), (r2, o, refs_o), (r3, t, refs_t), (r4, o, refs_o)):
            n.append(check_batch(r, w, refs, fig))
    finally:
        print(f"[window index] relative factor {factor}: windows 1, 2, 1, then index 1 of a new batch: worst {fig}, inf compared on {n}")
    for k in REL_KEYS:
        assert r1[k].tobytes() == r3[k].tobytes(), f"{k}: window 1 differs after a call on window 2"
        assert r2[k].tobytes() == r4[k].tobytes(), f"{k}: the same window at another index of another batch differs"


# ---- marginalize / sparsify --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", FACTORS)
def test_marginalize_vo_in_slot_1(backend_cls, oracle_lib, factor):
    t, args = bh.marg_vo_target(factor)
    assert len(args["lmk_keep"]) > 10 and len(args["lmk_marg"]) > 3
    a = bh.decoy(factor, "a")
    o = oracle_lib.marginalize(t, **args)
    be = backend_cls(device=0)
    try:
        be.set_windows([a, t])
        g1 = be.marginalize(1, **args)
        be.set_windows([t, a])
        g0 = be.marginalize(0, **args)
    finally:
        be.close()
    for g in (g1, g0):
        print(f"[window index] marginalize VO factor {factor}: |J^T J - oracle| / max {relerr(g['J'].T @ g['J'], o['J'].T @ o['J']):.3e}; bar 1e-8")
        check_prior(g, o)


def test_marginalize_and_sparsify_vio_in_slot_1(backend_cls, oracle_lib):
    t, args = bh.marg_vio_target()
    va = bh.decoy(PIXEL, "a", vio=True)
    o = oracle_lib.marginalize(t, **args)
    be = backend_cls(device=0)
    try:
        be.set_windows([va, t])
        g = be.marginalize(1, **args)
        fg = be.sparsify(1, g, vio=True)
    finally:
        be.close()
    print(f"[window index] marginalize VIO: |J^T J - oracle| / max {relerr(g['J'].T @ g['J'], o['J'].T @ o['J']):.3e}; bar 1e-8")
    assert g["kf_col"] == 0 and g["n"] == 15 + 3 * len(args["lmk_keep"])
    check_prior(g, o)
    fo = oracle_lib.sparsify(t, g, vio=True)                 # the same prior on both sides, as tests/test_gpu_sparsify.py::test_sparsify_vio
    worst = max(relerr(x["sqrt_inf"], y["sqrt_inf"]) for x, y in zip(fg, fo))
    print(f"[window index] sparsify VIO: {len(fg)} factors, worst |sqrt_inf - oracle| / max {worst:.3e}; bar 1e-7")
    same_factors(fg, fo)


def test_dense_prior_on_window_1_feeds_the_solve(backend_cls, oracle_lib):
    """tests/test_gpu_marg.py::test_device_prior_feeds_the_next_solve with both batches behind a VIO decoy; every window of the second
    batch against the oracle's solve of that window alone (the decoy: without any prior), at that test's bars."""
    w, args, w2 = bh.prior_pipeline_target()
    va, vb = bh.decoy(PIXEL, "a", vio=True), bh.decoy(PIXEL, "b", vio=True)
    keys = ("J", "r0", "kf_keep", "kf_col", "lmk_index", "lmk_col")
    opts = capi.reference_options()
    be = backend_cls(device=0)
    try:
        be.set_windows([va, w])
        g = be.marginalize(1, **args)
        w2.dense_prior = {k: g[k] for k in keys}
        be.set_windows([vb, w2])
        sums = be.solve(opts)
        ds = [be.get_deltas(0), be.get_deltas(1)]
    finally:
        be.close()
    o = oracle_lib.marginalize(w, **args)
    refs = [oracle_lib.solve(vb, opts), oracle_lib.solve(w2, opts, dense_prior={k: o[k] for k in keys})]
    for k, (s, d, ref) in enumerate(zip(sums, ds, refs)):
        rs = ref["summary"]
        print(f"[window index] dense prior, window {k}: cost {s.final_cost:.9e} (oracle {rs.final_cost:.9e}), iterations {s.iterations} ({rs.iterations}), "
              f"max |dpose| {np.abs(d['pose'] - ref['pose']).max():.2e} max |dlmk| {np.abs(d['lmk'] - ref['lmk']).max():.2e}; bars 1e-8, =, 1e-6, 1e-5")
        assert np.isclose(s.final_cost, rs.final_cost, rtol=1e-8)
        assert s.iterations == rs.iterations
        assert np.abs(d["pose"] - ref["pose"]).max() <= 1e-6 and np.abs(d["lmk"] - ref["lmk"]).max() <= 1e-5
    plain = oracle_lib.solve(w2, opts)                     # the prior matters on window 1 ...
    assert np.abs(plain["pose"] - refs[1]["pose"]).max() > 1e-6


# ---- covariance --------------------------------------------------------------------------------------------------------------------
def _opts():
    o = capi.reference_options()
    o.huber_a = 0.0
    return o


def test_covariance_of_windows_1_2_3(backend_cls):
    """One solve of [decoy, pixel_vo, lmk600, obs64]; covariance of windows 1, 2, 3 and again 3, 2, 1 (the scratch buffers are resized
    between windows of very different size): bit-identical passes, each window at tests/test_gpu_cov.py's bar for its own case
    (64 x E_REF). A batch takes the contiguous tile layout: k_cov_assemble's first run on it."""
    ws = [bh.decoy(PIXEL, "a"), ch.window_pixel_vo(), ch.window_lmk600(), ch.window_obs64()]
    req = {1: dict(kf=[0, 1, 2], pairs=[(0, 1), (1, 0)], lmk="all"), 2: dict(lmk="all"), 3: dict(kf=list(range(32)), pairs=[(0, 30)], lmk="all")}
    case = {1: "pixel_vo", 2: "lmk600", 3: "obs64"}
    be = backend_cls(device=0)
    try:
        be.set_windows(ws)
        be.solve(_opts())
        d = {k: be.get_deltas(k) for k in (1, 2, 3)}
        c1 = {k: be.covariance(k, **req[k]) for k in (1, 2, 3)}
        c2 = {k: be.covariance(k, **req[k]) for k in (3, 2, 1)}
        d_after = {k: be.get_deltas(k) for k in (1, 2, 3)}
    finally:
        be.close()
    for k in (1, 2, 3):
        info, _ = cov_check(case[k], ws[k], d[k], c1[k], pairs=req[k].get("pairs", ()), want_kf="kf" in req[k])
        for key in ("kf", "pair", "lmk"):
            assert c1[k][key].tobytes() == c2[k][key].tobytes(), (k, key)
        assert c1[k]["n_lmk_singular"] == c2[k]["n_lmk_singular"]
        for key in d[k]:
            assert d[k][key].tobytes() == d_after[k][key].tobytes(), (k, key)
    assert c1[1]["n_lmk_singular"] == 1 and np.isnan(c1[1]["lmk"][ch.SINGLE]).all() and np.all(c1[1]["kf"][2] == 0.0)
    assert c1[2]["kf"].shape[0] == 0 and c1[2]["lmk"].shape[0] == ws[2].n_lmk
    assert int(np.diff(ws[3].lmk_obs_ptr)[ch.OBS64_LMK]) == 64


def test_covariance_angular_window_1(backend_cls):
    ws = [bh.decoy(ANGULAR, "a"), ch.window_angular_vo()]
    pairs = [(0, 1), (0, 2), (1, 2)]
    be = backend_cls(device=0)
    try:
        be.set_windows(ws)
        be.solve(_opts())
        d = be.get_deltas(1)
        c = be.covariance(1, kf=list(range(4)), pairs=pairs, lmk="all")
    finally:
        be.close()
    cov_check("angular_vo", ws[1], d, c, pairs=pairs)


def test_covariance_vio_resident_prior_on_window_1(backend_cls):
    """tests/test_gpu_cov.py::test_vio_with_the_resident_prior (dense form) with both batches behind a VIO decoy."""
    w, args, w2, keep = ch.vio_marg_step()
    va = bh.decoy(PIXEL, "a", vio=True)
    be = backend_cls(device=0)
    try:
        be.set_prior(ch.VIO_J0, np.zeros(15))
        be.set_windows([va, w])
        g = be.marginalize(1, form="cholesky", readback=True, **args)
        assert g is not None and g["n_full"] == g["n"]
        w_ref = ch.vio_attach(w, w2, keep, g, None)
        w_dev = dataclasses.replace(w_ref, dense_prior=dict({k: v for k, v in w_ref.dense_prior.items() if k not in ("J", "r0")}, resident=True))
        be.set_windows([va, w_dev])
        be.solve(_opts())
        d = be.get_deltas(1)
        pairs = [(0, 3), (1, 2)]
        c = be.covariance(1, kf=list(range(4)), pairs=pairs, lmk="all")
    finally:
        be.close()
    assert c["kf"].shape == (4, 15, 15)
    cov_check("vio_dense", w_dev, d, c, pairs=pairs, w_ref=w_ref)


# ---- arguments ---------------------------------------------------------------------------------------------------------------------
def _sentinel(shape, dtype=np.float64):
    return np.full(shape, 7, dtype=dtype)


def test_arguments(backend_cls):
    """w == n_windows is refused by every entry point with its outputs untouched; an index that is in range for the decoy in front but
    not for the target (a key-frame >= 3, a landmark >= 40 of the 3-KF / 40-landmark covariance window behind the 7-KF / 90-landmark
    decoy) is refused on the TARGET's sizes."""
    a, t = bh.decoy(PIXEL, "a"), ch.window_pixel_vo()
    assert t.n_kf < 5 < a.n_kf and t.n_lmk < 60 < a.n_lmk
    E = capi.E_INVALID_ARG
    be = backend_cls(device=0)
    lib = be.lib
    try:
        be.set_windows([a, t])
        be.solve(_opts())

        def linearize(w):
            r, Jp, Jl = _sentinel(2 * t.n_obs), _sentinel(12 * t.n_obs), _sentinel(6 * t.n_obs)
            rc = lib.sadvio_ba_linearize(be.h, w, _dp(), _dp(), r.ctypes.data_as(_dp), Jp.ctypes.data_as(_dp), Jl.ctypes.data_as(_dp))
            return rc, bool((r == 7).all() and (Jp == 7).all() and (Jl == 7).all())

        def chi2(w):
            avg, inl = _sentinel(t.n_lmk), _sentinel(t.n_lmk, np.int32)
            rc = lib.sadvio_ba_landmark_chi2(be.h, w, _dp(), _dp(), _dp(), 0.0, avg.ctypes.data_as(_dp), inl.ctypes.data_as(_ip))
            return rc, bool((avg == 7).all() and (inl == 7).all())

        def relative(w, p, q):
            inf, Ak = _sentinel(36), _sentinel(144)
            rc = lib.sadvio_ba_marginalize_relative(be.h, w, p, q, 1, inf.ctypes.data_as(_dp), Ak.ctypes.data_as(_dp))
            return rc, bool((inf == 7).all() and (Ak == 7).all())

        def marginalize(w, kf_marg=2, kf_keep=-1, marg=(0, 1), keep=(2, 3, 4)):
            rq = capi.MargRequestC()
            mk, kp = np.array(marg, dtype=np.int32), np.array(keep, dtype=np.int32)
            rq.kf_marg, rq.kf_keep, rq.n_marg, rq.lmk_marg, rq.n_keep, rq.lmk_keep = kf_marg, kf_keep, len(mk), mk.ctypes.data_as(_ip), len(kp), kp.ctypes.data_as(_ip)
            rq.eig_cut_mode = 1
            res = capi.MargResultC(7, 7, 7, 7, 7, 7)
            col, J, r0 = _sentinel(len(kp), np.int32), _sentinel(81), _sentinel(9)
            rc = lib.sadvio_ba_marginalize(be.h, w, C.byref(rq), C.byref(res), col.ctypes.data_as(_ip), J.ctypes.data_as(_dp), r0.ctypes.data_as(_dp))
            return rc, bool((col == 7).all() and (J == 7).all() and (r0 == 7).all() and (res.m, res.n, res.n_full, res.kf_col) == (7, 7, 7, 7))

        def sparsify(w, kf_keep=1, lmk=(2, 3)):
            n = 15 + 3 * len(lmk)
            J = np.eye(n)
            li = np.array(lmk, dtype=np.int32); lc = (15 + 3 * np.arange(len(lmk))).astype(np.int32)
            out = (capi.SparsePriorC * (len(lmk) + 1))()
            for s in out:
                s.type = 7
            n_out = C.c_int32(7)
            rc = lib.sadvio_ba_sparsify(be.h, w, 1, n, n, J.ctypes.data_as(_dp), kf_keep, 0, len(li), li.ctypes.data_as(_ip), lc.ctypes.data_as(_ip), C.byref(n_out), out)
            return rc, all(s.type == 7 for s in out) and n_out.value in (0, 7)      # (n_out is cleared on entry, as sadvio_ba.h says)

        def dense_prior(w, kf_keep=-1, lmk=(2, 3)):
            n = (15 if kf_keep >= 0 else 0) + 3 * len(lmk)
            J, r0 = np.eye(n), np.zeros(n)
            li = np.array(lmk, dtype=np.int32); lc = ((15 if kf_keep >= 0 else 0) + 3 * np.arange(len(lmk))).astype(np.int32)
            return lib.sadvio_ba_set_dense_prior(be.h, w, n, n, J.ctypes.data_as(_dp), r0.ctypes.data_as(_dp), kf_keep, 0, len(li), li.ctypes.data_as(_ip), lc.ctypes.data_as(_ip))

        def cov(w, **kw):
            r = be.covariance(w, raw_rc=True, **kw)
            return r["rc"], bool(np.all(r["kf"] == 0.0) and np.all(r["pair"] == 0.0) and np.all(r["lmk"] == 0.0))

        # w == n_windows
        assert cov(2, kf=[0], pairs=[(0, 1)], lmk=[0]) == (E, True)
        assert raw_call(be, 2, [0], [1]) == (E, True)
        assert relative(2, 0, 1) == (E, True)
        assert marginalize(2) == (E, True)
        assert sparsify(2) == (E, True)
        assert chi2(2) == (E, True)
        assert linearize(2) == (E, True)
        assert dense_prior(2) == E
        # in range for the decoy, out of range for the target
        for kw in (dict(kf=[5]), dict(kf=[3]), dict(pairs=[(0, 5)]), dict(pairs=[(3, 0)]), dict(lmk=[60]), dict(lmk=[40])):
            assert cov(1, **kw) == (E, True), kw
        for p, q in ((0, 5), (5, 0), (3, 1), (1, 3)):
            assert raw_call(be, 1, [0, p], [1, q]) == (E, True), (p, q)
            assert relative(1, p, q) == (E, True), (p, q)
        for kw in (dict(kf_marg=5), dict(kf_marg=3), dict(kf_keep=5), dict(kf_keep=3), dict(marg=(0, 60)), dict(marg=(40,)), dict(keep=(2, 3, 60)), dict(keep=(2, 3, 40))):
            assert marginalize(1, **kw) == (E, True), kw
        for kw in (dict(kf_keep=5), dict(kf_keep=3), dict(lmk=(2, 60)), dict(lmk=(40, 3))):
            assert sparsify(1, **kw) == (E, True), kw
        for kw in (dict(kf_keep=5), dict(kf_keep=3), dict(lmk=(2, 60)), dict(lmk=(40, 3))):
            assert dense_prior(1, **kw) == E, kw
        # ... and the same indices are accepted where they are in range: the decoy itself
        assert cov(0, kf=[5], pairs=[(0, 5)], lmk=[60])[0] == OK
        assert raw_call(be, 0, [0, 5], [1, 0])[0] == OK
        assert relative(0, 5, 4)[0] in (OK, REFUSED)
        # the refused calls changed nothing: the target still answers, at the bar of its own test
        d = be.get_deltas(1)
        c = be.covariance(1, kf=[0, 1, 2], pairs=[(0, 1)], lmk="all")
    finally:
        be.close()
    cov_check("pixel_vo", t, d, c, pairs=[(0, 1)])
