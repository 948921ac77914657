"""sadvio_ba_covariance_batch on the device. The reference and the bar are those of tests/test_gpu_cov.py: blocks of np.linalg.inv of
the FULL information matrix (tests/cov_helpers.py) at the deltas the device's own solve returned; a block passes at TOL_FACTOR = 64 x
E_REF of its window (tests/cov_batch_helpers.py: the recorded yardsticks, and the five new windows measured by
tests/test_cov_batch_cpu.py). On the DENSE and NONE routes an item must carry the bits of sadvio_ba_covariance on the same handle;
on the LDS route (S inverted inside one workgroup's LDS, another factorisation order) it must meet the bar. Every case prints its
worst figure before it asserts.
"""
import dataclasses

import numpy as np
import pytest

import batch_helpers as bh
import cov_batch_helpers as cb
import cov_helpers as ch
from sadvio_amd import capi, synthetic

pytestmark = pytest.mark.gpu

NONE, LDS, DENSE = capi.COV_ROUTE_NONE, capi.COV_ROUTE_LDS, capi.COV_ROUTE_DENSE
PIXEL, ANGULAR = capi.FACTOR_PIXEL, capi.FACTOR_ANGULAR
SENTINEL = 7.0


def _opts(huber=0.0, iters=None):
    o = capi.reference_options()
    o.huber_a = huber
    if iters is not None:
        o.max_num_iterations = iters
    return o


def _single(be, it):
    return be.covariance(it["w"], kf=it.get("kf"), pairs=it.get("pairs"), lmk=it.get("lmk"))


# ---- the pixel batch of cases 1, 10, 11, 12 -------------------------------------------------------------------------------------------
PIX_CASE = {1: "pixel_vo", 2: "lmk600", 3: "obs64"}
PIX_ITEMS = [dict(w=3, kf=list(range(32)), pairs=[(0, 30)], lmk="all"),
             dict(w=1, kf=[0, 1, 2], pairs=[(0, 1), (1, 0)], lmk="all"),
             dict(w=2, lmk="all"),
             dict(w=1, lmk=[5, ch.SINGLE, 5])]


def _pixel_windows():
    return [bh.decoy(PIXEL, "a"), ch.window_pixel_vo(), ch.window_lmk600(), ch.window_obs64()]


def _run_pixel(backend_cls, with_single=False):
    ws = _pixel_windows()
    be = backend_cls(device=0)
    try:
        be.set_windows(ws)
        be.solve(_opts())
        d = {k: be.get_deltas(k) for k in (1, 2, 3)}
        got = be.covariance_batch(PIX_ITEMS)
        solo = [be.covariance_batch([it])[0] for it in PIX_ITEMS]               # every item in a call, hence a group, of its own
        single = [_single(be, it) for it in PIX_ITEMS] if with_single else None
    finally:
        be.close()
    return ws, d, got, single, solo


@pytest.fixture(scope="module")
def pixel_default(backend_cls):
    return _run_pixel(backend_cls, with_single=True)


def test_pixel_batch(pixel_default):
    """Case 1: [decoy, pixel_vo, lmk600, obs64], items on windows 3, 1, 2 and again 1 (a landmark selection only)."""
    ws, d, got, single, _ = pixel_default
    assert [g["route"] for g in got] == [DENSE, LDS, LDS, LDS] and all(g["status"] == 0 for g in got)
    assert cb.n_p(ws[1]) == 12 and cb.n_p(ws[2]) == 42 and cb.n_p(ws[3]) == 186
    for it, g in zip(PIX_ITEMS, got):
        cb.check_item(PIX_CASE[it["w"]], ws[it["w"]], d[it["w"]], g, pairs=it.get("pairs", ()), kf=it.get("kf"), lmk=it.get("lmk"))
    assert cb.same_bytes(got[0], single[0])                                   # the dense route: the single call's bits
    assert got[1]["n_lmk_singular"] == 1 and np.isnan(got[1]["lmk"][ch.SINGLE]).all() and np.all(got[1]["kf"][2] == 0.0)
    assert np.array_equal(got[1]["pair"][0], got[1]["pair"][1].T)
    for k in range(2):
        assert np.array_equal(got[1]["kf"][k], got[1]["kf"][k].T) and np.all(np.linalg.eigvalsh(got[1]["kf"][k]) > 0)
    assert got[3]["kf"].shape[0] == 0 and got[3]["n_lmk_singular"] == 1 and np.isnan(got[3]["lmk"][1]).all()
    assert got[3]["lmk"][0].tobytes() == got[1]["lmk"][5].tobytes() == got[3]["lmk"][2].tobytes()
    worst = max(cb.worst_difference(g, s) for g, s in zip(got[1:], single[1:]))
    print(f"[cov batch] pixel batch: LDS items against the single calls, worst relative block difference {worst:.3e}")


def test_angular_batch(backend_cls):
    """Case 2: N_p = 18 crosses the 16-column tile of the in-LDS factorisation; all cross pairs."""
    ws = [bh.decoy(ANGULAR, "a"), ch.window_angular_vo()]
    pairs = [(a, b) for a in range(3) for b in range(3) if a != b]
    be = backend_cls(device=0)
    try:
        be.set_windows(ws)
        be.solve(_opts())
        d = be.get_deltas(1)
        got = be.covariance_batch([dict(w=1, kf=list(range(4)), pairs=pairs, lmk="all")])[0]
    finally:
        be.close()
    assert got["route"] == LDS and got["status"] == 0 and cb.n_p(ws[1]) == 18
    cb.check_item("angular_vo", ws[1], d, got, pairs=pairs, kf=list(range(4)))
    assert np.all(got["kf"][3] == 0.0)


@pytest.mark.parametrize("form", ["dense", "sparse"])
def test_vio_with_the_resident_prior(backend_cls, form):
    """Case 3: the VIO window of tests/test_gpu_cov.py behind a VIO decoy: 15 x 15 blocks, N_p = 4 x 15 + 3 x 5 kept landmarks."""
    w, args, w2, keep = ch.vio_marg_step()
    va = bh.decoy(PIXEL, "a", vio=True)
    be = backend_cls(device=0)
    try:
        be.set_prior(ch.VIO_J0, np.zeros(15))
        be.set_windows([va, w])
        g = be.marginalize(1, form="cholesky", readback=True, **args)
        assert g is not None and g["n_full"] == g["n"]
        resident = {k: v for k, v in g.items() if k not in ("J", "r0")}
        resident["resident"] = True
        fs = be.sparsify(1, resident, vio=True) if form == "sparse" else None
        w_ref = ch.vio_attach(w, w2, keep, g, fs)
        w_dev = w_ref
        if form == "dense":
            w_dev = dataclasses.replace(w_ref, dense_prior=dict({k: v for k, v in w_ref.dense_prior.items() if k not in ("J", "r0")}, resident=True))
        be.set_windows([va, w_dev])
        be.solve(_opts())
        d = be.get_deltas(1)
        pairs = [(0, 3), (1, 2)]
        c = be.covariance_batch([dict(w=1, kf=list(range(4)), pairs=pairs, lmk="all")])[0]
    finally:
        be.close()
    assert c["kf"].shape == (4, 15, 15) and c["route"] == LDS and c["status"] == 0
    cb.check_item("vio_" + form, w_dev, d, c, pairs=pairs, kf=list(range(4)), w_ref=w_ref)
    kept = [int(np.flatnonzero(w_ref.lmk_id == w.lmk_id[l])[0]) for l in keep if len(np.flatnonzero(w_ref.lmk_id == w.lmk_id[l]))]
    assert len(kept) >= 1 and all(np.isfinite(c["lmk"][l]).all() and np.all(np.linalg.eigvalsh(c["lmk"][l]) > 0) for l in kept)


def test_huber(backend_cls):
    """Case 4: the corrector of the last solve is applied to every item."""
    ws = [ch.window_huber(), ch.window_pixel_vo()]
    item = dict(w=0, kf=[0, 1, 2], pairs=[(0, 1)], lmk="all")
    res = {}
    for huber in (ch.HUBER_A, 0.0):
        be = backend_cls(device=0)
        try:
            be.set_windows(ws)
            be.solve(_opts(huber))
            res[huber] = (be.get_deltas(0), be.covariance_batch([item, dict(w=1, kf=[0])])[0])
        finally:
            be.close()
    d, c = res[ch.HUBER_A]
    assert c["route"] == LDS
    cb.check_item("huber", ws[0], d, c, huber=ch.HUBER_A, pairs=[(0, 1)], kf=[0, 1, 2])
    moved = ch.rel_diff(c["kf"][0], res[0.0][1]["kf"][0])
    print(f"[cov batch] huber: block (0, 0) against the same item without loss: {moved:.3e}")
    assert moved > 1e-3


def test_cap_boundary(backend_cls):
    """Case 5: N_p = 174 is the largest window of these tests on the LDS route, 180 the smallest on the dense one."""
    ws = [cb.window("np174"), cb.window("np180")]
    items = [dict(w=0, kf=list(range(30)), pairs=[(0, 28), (28, 0)], lmk="all"), dict(w=1, kf=list(range(31)), pairs=[(0, 29)], lmk="all")]
    be = backend_cls(device=0)
    try:
        be.set_windows(ws)
        be.solve(_opts())
        d = [be.get_deltas(k) for k in range(2)]
        got = be.covariance_batch(items)
        single = _single(be, items[1])
    finally:
        be.close()
    assert [g["route"] for g in got] == [LDS, DENSE] and cb.n_p(ws[0]) == 174 and cb.n_p(ws[1]) == 180
    cb.check_item("np174", ws[0], d[0], got[0], pairs=items[0]["pairs"], kf=items[0]["kf"])
    cb.check_item("np180", ws[1], d[1], got[1], pairs=items[1]["pairs"], kf=items[1]["kf"])
    assert cb.same_bytes(got[1], single)
    assert np.array_equal(got[0]["pair"][0], got[0]["pair"][1].T)


@pytest.mark.parametrize("cases", [("w7", "w42"), ("w7_angular", "w7_angular")])
def test_after_the_throughput_kernels(backend_cls, monkeypatch, cases):
    """Case 6: a batch k_lm_pass solved, stopped after two iterations: the two delta buffers differ by a whole step, so a covariance
    linearised at the wrong one misses the bar at get_deltas' deltas. The single call keeps refusing such a batch."""
    monkeypatch.setenv("SADVIO_LM", "1")
    ws = [cb.window(c) for c in cases]
    items = [dict(w=k, kf=list(range(ws[k].n_kf)), pairs=[(0, 3)], lmk="all") for k in range(2)]
    be = backend_cls(device=0, profile_kernels=True)
    try:
        be.set_windows(ws)
        s = be.solve(_opts(iters=2))
        times = be.kernel_times()
        d = [be.get_deltas(k) for k in range(2)]
        r = be.covariance(0, kf=[0], raw_rc=True)
        got = be.covariance_batch(items)
    finally:
        be.close()
    assert "k_lm_pass" in times and "k_backsub" not in times, sorted(times)
    assert all(x.iterations == 2 for x in s)
    assert r["rc"] == capi.E_INVALID_ARG and "throughput" in r["error"]
    for k in range(2):
        assert got[k]["route"] == LDS and got[k]["status"] == 0
        cb.check_item(cases[k], ws[k], d[k], got[k], pairs=[(0, 3)], kf=items[k]["kf"], tag=" after k_lm_pass")


def test_per_item_status(backend_cls):
    """Case 7: the unanchored window of tests/test_gpu_cov.py beside a well-posed one."""
    wu = synthetic.make_window(n_kf=4, n_lmk=60, obs_per_lmk=4, seed=33, fixed=0)
    wu.pose_priors = []
    ws = [ch.window_pixel_vo(), wu]
    items = [dict(w=1, kf=[0, 1], pairs=[(0, 1)], lmk="all"), dict(w=0, kf=[0, 1, 2], pairs=[(0, 1)], lmk="all"), dict(w=1, lmk=[3])]
    be = backend_cls(device=0)
    try:
        be.set_windows(ws)
        be.solve(_opts())
        d = be.get_deltas(0)
        got = be.covariance_batch(items, fill=SENTINEL)
    finally:
        be.close()
    for g in (got[0], got[2]):
        assert g["status"] == capi.E_NOT_USABLE and g["route"] == LDS
        assert np.all(g["kf"] == SENTINEL) and np.all(g["pair"] == SENTINEL) and np.all(g["lmk"] == SENTINEL)
    assert got[1]["status"] == 0
    cb.check_item("pixel_vo", ws[0], d, got[1], pairs=[(0, 1)], kf=[0, 1, 2])


def test_every_key_frame_constant(backend_cls):
    """Case 8: N_p = 0, Sigma_ll = H_ll^-1."""
    from frontend_helpers import landmark_optimization_window
    ws = [landmark_optimization_window(), ch.window_pixel_vo()]
    items = [dict(w=0, kf=[0, 1], pairs=[(0, 1)], lmk="all"), dict(w=1, kf=[0])]
    be = backend_cls(device=0)
    try:
        be.set_windows(ws)
        be.solve(_opts(ch.HUBER_A))
        got = be.covariance_batch(items)
        single = _single(be, items[0])
    finally:
        be.close()
    assert got[0]["route"] == NONE and got[0]["status"] == 0 and got[1]["route"] == LDS
    assert cb.same_bytes(got[0], single)
    ok = ~np.isnan(got[0]["lmk"]).any(axis=(1, 2))
    print(f"[cov batch] N_p = 0: {int(ok.sum())} of {len(ok)} landmark blocks finite, byte-identical to the single call")
    assert ok.sum() > 0.9 * len(ok) and np.all(got[0]["kf"] == 0.0) and np.all(got[0]["pair"] == 0.0)


def test_contract(backend_cls):
    """Case 9: the setups of tests/test_gpu_cov.py::test_refusals."""
    from line_helpers import add_lines
    from sadvio_amd import sharding
    w = ch.window_angular_vo()
    be = backend_cls(device=0)
    try:
        be.set_windows([w])
        r = be.covariance_batch([dict(w=0, kf=[0])], raw_rc=True)
        assert r["rc"] == capi.E_STATE and "before solve" in r["error"]
        be.solve(_opts())
        assert be.covariance_batch([]) == []
        good = dict(w=0, kf=[0, 1], pairs=[(0, 1)], lmk="all")
        for bad in (dict(w=0, kf=[4]), dict(w=0, kf=[-1]), dict(w=0, pairs=[(0, 9)]), dict(w=0, lmk=[w.n_lmk]), dict(w=0, lmk=[-2]), dict(w=1, kf=[0]),
                    dict(w=-1, kf=[0])):
            r = be.covariance_batch([good, good, bad], raw_rc=True, fill=SENTINEL)
            assert r["rc"] == capi.E_INVALID_ARG and "out of range" in r["error"], bad
            for o in r["items"][:2]:
                assert np.all(o["kf"] == SENTINEL) and np.all(o["pair"] == SENTINEL) and np.all(o["lmk"] == SENTINEL), bad
        assert be.lib.sadvio_ba_covariance_batch(be.h, -1, None) == capi.E_INVALID_ARG
        assert be.lib.sadvio_ba_covariance_batch(be.h, 1, None) == capi.E_INVALID_ARG
        be._check(be.lib.sadvio_ba_begin_update(be.h), "begin_update")
        r = be.covariance_batch([good], raw_rc=True)
        be._check(be.lib.sadvio_ba_commit_update(be.h), "commit_update")
        assert r["rc"] == capi.E_STATE and "begin_update" in r["error"]
    finally:
        be.close()
    wl = add_lines(synthetic.make_window(n_kf=4, n_lmk=60, obs_per_lmk=4, seed=21), n_line=3, obs_per_line=4)
    be = backend_cls(device=0)
    try:
        be.set_windows([wl]); be.solve(_opts())
        r = be.covariance_batch([dict(w=0, kf=[0])], raw_rc=True)
        assert r["rc"] == capi.E_INVALID_ARG and "line landmarks" in r["error"]
    finally:
        be.close()
    be = backend_cls(device=0)
    try:
        be.set_collective(0, 2, lambda *a: 0)
        be.set_windows([sharding.shard_window(synthetic.make_window(n_kf=5, n_lmk=300, seed=42), 0, 2)])
        r = be.covariance_batch([dict(w=0, kf=[0])], raw_rc=True)
        assert r["rc"] == capi.E_INVALID_ARG and "sharded" in r["error"]
    finally:
        be.close()


def test_untouched_and_deterministic(backend_cls, pixel_default):
    """Case 10: the solve's results keep their bytes; two calls agree to the bit; an item's bits do not depend on its neighbours or on
    its position."""
    ws = _pixel_windows()
    it = {k: next(i for i in PIX_ITEMS if i["w"] == k) for k in (1, 2, 3)}
    be = backend_cls(device=0)
    try:
        be.set_windows(ws)
        be.solve(_opts())
        d0 = {k: be.get_deltas(k) for k in range(4)}
        t0 = {k: be.get_trace(k) for k in range(4)}
        a = be.covariance_batch([it[1], it[2]])
        d1 = {k: be.get_deltas(k) for k in range(4)}
        t1 = {k: be.get_trace(k) for k in range(4)}
        b = be.covariance_batch([it[1], it[2]])
        c = be.covariance_batch([it[2], it[3], it[1]])
    finally:
        be.close()
    for k in range(4):
        assert t0[k].tobytes() == t1[k].tobytes()
        for key in d0[k]:
            assert d0[k][key].tobytes() == d1[k][key].tobytes(), (k, key)
    assert cb.same_bytes(a[0], b[0]) and cb.same_bytes(a[1], b[1])
    assert cb.same_bytes(a[0], c[2]) and cb.same_bytes(a[1], c[0])
    # ... nor on the handle, where its solve returned the same bits: the module's default run asked for the same items among others
    _, d_def, got, _, _ = pixel_default
    for k, mine, theirs in ((1, a[0], got[1]), (2, a[1], got[2]), (3, c[1], got[0])):
        same_d = all(d0[k][key].tobytes() == d_def[k][key].tobytes() for key in d0[k])
        same_c = cb.same_bytes(mine, theirs)
        print(f"[cov batch] window {k} on a second handle: deltas bit-identical {same_d}, covariances bit-identical {same_c}, "
              f"worst relative block difference {cb.worst_difference(mine, theirs):.3e}")
        if same_d:
            assert same_c, k


def test_groups(backend_cls, monkeypatch, pixel_default):
    """Case 11: under a scratch budget of 1 MiB pixel_vo and lmk600 (1.09 MB of work arrays) cannot share a group. Grouping must not
    change a bit. Two handles do not solve to the same bits (the solve's own sums are not ordered: the deltas of two runs differ in the
    last places, measured here 1e-12 relative on the covariances), so the comparison is made where the state is the same: on each
    handle, the call that holds all items against calls of one item — one window, one group — each. That holds on the default
    handle (windows 1 and 2 share a group) and on the small-budget handle (they cannot), which is what invariance under grouping means.
    Where the second handle's solve does return the default run's bits, so must the call."""
    ws, d, got, _, solo = pixel_default
    for g, one in zip(got, solo):
        assert g["route"] == one["route"] and cb.same_bytes(g, one)
    monkeypatch.setenv("SADVIO_COV_BATCH_SCRATCH_MB", "1")
    ws2, d2, got2, _, solo2 = _run_pixel(backend_cls)
    assert cb.unit_bytes(ws2[2]) > (1 << 20)                                  # window 2 alone is over the budget: at least two groups
    same_d = all(d2[k][key].tobytes() == d[k][key].tobytes() for k in d for key in d[k])
    worst = max(cb.worst_difference(g, ref) for g, ref in zip(got2, got))
    print(f"[cov batch] groups: second handle's deltas bit-identical to the default run's {same_d}; items against the default run's, "
          f"worst relative block difference {worst:.3e}")
    for g, one, ref in zip(got2, solo2, got):
        assert g["route"] == ref["route"] and cb.same_bytes(g, one)
        if same_d:
            assert cb.same_bytes(g, ref)


def test_route_ab(backend_cls, monkeypatch, pixel_default):
    """Case 12: SADVIO_COV_BATCH_LDS=0 sends every item down the dense route, with the single call's bits; the LDS run of the same
    items lies within the sum of the two bars."""
    monkeypatch.setenv("SADVIO_COV_BATCH_LDS", "0")
    ws, d, got, single, _ = _run_pixel(backend_cls, with_single=True)
    assert all(g["route"] == DENSE and g["status"] == 0 for g in got)
    for g, s in zip(got, single):
        assert cb.same_bytes(g, s)
    for it, g, lds in zip(PIX_ITEMS, got, pixel_default[2]):
        worst = cb.worst_difference(lds, g)
        bar = 2 * ch.TOL_FACTOR * cb.E_REF[PIX_CASE[it["w"]]]
        print(f"[cov batch] window {it['w']} ({PIX_CASE[it['w']]}): LDS run against dense run {worst:.3e}; bound {bar:.3e}")
        assert worst <= bar
