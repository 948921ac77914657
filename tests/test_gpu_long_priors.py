"""Long tracks (landmarks of more than 64 observations) under priors, on the device: handles created with SADVIO_CFG_LONG_TRACKS |
SADVIO_CFG_LONG_TRACK_PRIORS (capi.Backend(long_tracks=True, long_track_priors=True)) marginalise, sparsify and keep them in the
reduced system. Windows, references and bars: tests/long_prior_helpers.py.

  1. marginalize    KL65 and KMIX against oracle.marginalize (check_prior of test_gpu_marg.py, rtol 1e-8); KMIX with a long track moved
                    from lmk_keep to lmk_marg; KMIX on top of the handle's resident prior
  2. first step     one LM step under the prior that keeps the long tracks against the 50-digit step, at TOL_FACTOR x max(E_REF, FLOOR);
                    model cost change and cost after the step to 1e-11 (the bar of test_gpu_long_tracks.py)
  3. pipelines      marginalize -> set_dense_prior(resident) -> solve and marginalize -> sparsify -> set_sparse_priors -> solve on KMIX
                    against the same pipelines on the oracle. Under the reference's options the dense-prior solve of KMIX rejects ten
                    steps: the candidate of a kept long track survives a rejection. KVIO (15 states per key-frame): marginalize with
                    kf_keep, the IMU factor and a previous prior, and the sparsified VIO pipeline, whose pose-to-landmark factor holds
                    the long track. A pose-to-landmark factor on a free long track (KMIX; a 15-state window) against the oracle
  4. graph         use_graph = 1: KMIX with its long tracks free, kept by the prior, free again, on ONE handle
  5. flags          bit 2 alone is refused at create; bit 1 alone keeps every refusal; both bits: the covariance family and the
                    relative marginalisations still refuse and leave the solved state alone

Every case prints its figures (`LONGPRIOR ...`, run with -s) before it asserts."""
import numpy as np
import pytest

import long_prior_helpers as ph
import long_track_helpers as lh
import step_helpers as sh
from sadvio_amd import capi
from test_gpu_marg import check_prior
from test_gpu_sparsify import same_factors

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _no_switch(monkeypatch):
    for k in sh.SWITCHES + ("SADVIO_LONG_MIN",):
        monkeypatch.delenv(k, raising=False)


def backend(backend_cls, **kw):
    return backend_cls(device=0, long_tracks=True, long_track_priors=True, **kw)


# ---- 1. marginalize ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["KL65", "KMIX"])
def test_marginalize_a_window_with_long_tracks(backend_cls, oracle_lib, name):
    w = ph.case_window(ph.CASE[name])
    args = ph.marg_args(w)
    assert set(args["lmk_keep"]) & set(lh.long_landmarks(w).tolist())
    be = backend(backend_cls)
    try:
        be.set_windows([w])
        g = be.marginalize(0, **args)
    finally:
        be.close()
    o = oracle_lib.marginalize(w, **args)
    print(f"LONGPRIOR marginalize {name}: m {g['m']} n {g['n']} n_full {g['n_full']} kept {args['lmk_keep']}")
    check_prior(g, o)


def test_marginalize_with_a_long_track_marginalised_and_on_a_resident_prior(backend_cls, oracle_lib):
    w = ph.case_window(ph.CASE["KMIX"])
    args = ph.marg_args(w)
    long_kept = [l for l in args["lmk_keep"] if l in lh.long_landmarks(w)]
    moved = dict(args, lmk_keep=[l for l in args["lmk_keep"] if l != long_kept[0]], lmk_marg=args["lmk_marg"] + [long_kept[0]])
    be = backend(backend_cls)
    try:
        be.set_windows([w])
        g_moved = be.marginalize(0, **moved)
        g1 = be.marginalize(0, **args)                               # the handle's prior from here on
        last = {k: g1[k] for k in ("kf_keep", "kf_col", "lmk_index", "lmk_col")}
        g2 = be.marginalize(0, **dict(args, last=last))              # last without "J": SADVIO_PRIOR_RESIDENT
    finally:
        be.close()
    check_prior(g_moved, oracle_lib.marginalize(w, **moved))
    o1 = oracle_lib.marginalize(w, **args)
    check_prior(g1, o1)
    check_prior(g2, oracle_lib.marginalize(w, **dict(args, last={k: o1[k] for k in ph.PRIOR_KEYS})))


# ---- 2. the first step under a prior that keeps long tracks ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ph.CASES, ids=[c.name for c in ph.CASES])
def test_first_step_with_kept_long_tracks_against_50_digits(backend_cls, oracle_lib, case):
    w = ph.case_prior_window(case, oracle_lib)
    ref = ph.reference(case, oracle_lib)
    be = backend(backend_cls, profile_kernels=True)
    try:
        be.set_windows([w])
        s = be.solve(ph.case_options(case))[0]
        d, tr, kt = be.get_deltas(0), be.get_trace(0), be.kernel_times()
    finally:
        be.close()
    n = {k: v["launches"] for k, v in kt.items()}
    assert n.get("k_long_lin") == 1 and n.get("k_long_back") == 1 and n.get("k_build_kept") == 1, n
    if case.name == "KBIG":                                          # the reduced system with the prior's columns leaves LDS
        assert sh.reduced_np(w) == 249 > sh.MAX_LDS_NP and "k_solve_front" in n and "k_solve" not in n, n
    if case.name == "K258":                                          # more observations than a workgroup of the long kernels has threads
        assert lh.counts(w).min() == 258 > 256
    e = sh.step_error(d, ref, w)
    unit = [max(v, sh.FLOOR) for v in ph.E_REF[case.window]]
    mcc_rel, cost_rel = abs(tr[1][7] / ref["model_cost_change"] - 1), abs(tr[1][0] / ref["cost"] - 1)
    print(f"LONGPRIOR first step {case.name}: Np {sh.reduced_np(w)} multiple pose {e[0] / unit[0]:.2f} lmk {e[1] / unit[1]:.2f} "
          f"(bar {sh.TOL_FACTOR:.0f}) mcc {mcc_rel:.1e} cost {cost_rel:.1e} steps {s.num_successful_steps}")
    assert s.num_successful_steps == 1
    bar_p, bar_l = ph.bars(case)
    assert e[0] <= bar_p, ("pose part", e[0], bar_p)
    assert e[1] <= bar_l, ("landmark part", e[1], bar_l)
    assert np.isclose(tr[1][7], ref["model_cost_change"], rtol=1e-11, atol=0)
    assert np.isclose(tr[1][0], ref["cost"], rtol=1e-11, atol=0)
    kept_long = [int(l) for l, c in zip(w.dense_prior["lmk_index"], w.dense_prior["lmk_col"]) if c >= 0 and l in lh.long_landmarks(w)]
    assert len(kept_long) == case.n_keep_long and np.abs(d["lmk"][kept_long]).min() > 0      # the kept long tracks moved


def test_window_1_of_a_batch_behind_a_decoy(backend_cls, oracle_lib):
    """KMIX at index 1 behind a decoy window of batch_helpers: marginalize(1) against the oracle, then the first step of window 1 under
    the prior that keeps its long tracks at the 50-digit bar (kept list, lmk_red and the long list carry the window's bases)."""
    import batch_helpers as bh
    case = ph.CASE["KMIX"]
    w, wp = ph.case_window(case), ph.case_prior_window(case, oracle_lib)
    args = ph.marg_args(w)
    a = bh.decoy(lh.PIXEL, "a")
    be = backend(backend_cls)
    try:
        be.set_windows([a, w])
        g = be.marginalize(1, **args)
        be.set_windows([a, wp])
        s = be.solve(ph.case_options(case))[1]
        d, tr = be.get_deltas(1), be.get_trace(1)
    finally:
        be.close()
    check_prior(g, oracle_lib.marginalize(w, **args))
    ref = ph.reference(case, oracle_lib)
    e = sh.step_error(d, ref, wp)
    bar_p, bar_l = ph.bars(case)
    print(f"LONGPRIOR KMIX@1 behind a decoy: pose {e[0] / bar_p * sh.TOL_FACTOR:.2f} lmk {e[1] / bar_l * sh.TOL_FACTOR:.2f} of the unit (bar {sh.TOL_FACTOR:.0f})")
    assert s.num_successful_steps == 1 and e[0] <= bar_p and e[1] <= bar_l
    assert np.isclose(tr[1][7], ref["model_cost_change"], rtol=1e-11, atol=0) and np.isclose(tr[1][0], ref["cost"], rtol=1e-11, atol=0)


# ---- 3. the pipelines ------------------------------------------------------------------------------------------------------------------------
def _compare_solve(tag, s, d, ref):
    rs = ref["summary"]
    ep, el = np.abs(d["pose"] - ref["pose"]).max(), np.abs(d["lmk"] - ref["lmk"]).max()
    print(f"LONGPRIOR {tag}: iterations {s.iterations} / {rs.iterations} unsuccessful {s.num_unsuccessful_steps} / {rs.num_unsuccessful_steps} "
          f"final cost {s.final_cost:.12g} / {rs.final_cost:.12g} pose {ep:.2e} lmk {el:.2e}")
    print(f"LONGPRIOR {tag}: final cost relative difference {abs(s.final_cost / rs.final_cost - 1):.1e}")
    return rs, ep, el


def test_pipeline_marginalize_resident_prior_solve(backend_cls, oracle_lib):
    w = ph.case_window(ph.CASE["KMIX"])
    args = ph.marg_args(w)
    opts = capi.reference_options()
    be = backend(backend_cls)
    try:
        be.set_windows([w])
        g = be.marginalize(0, readback=False, **args)
        assert g.get("J") is None
        be.set_windows([ph.next_window(w, g)])                       # resident: the prior never leaves the device
        s = be.solve(opts)[0]
        d = be.get_deltas(0)
    finally:
        be.close()
    o = oracle_lib.marginalize(w, **args)
    ref = oracle_lib.solve(w, opts, dense_prior={k: o[k] for k in ph.PRIOR_KEYS})
    rs, ep, el = _compare_solve("marginalize -> resident prior -> solve KMIX", s, d, ref)
    assert rs.num_unsuccessful_steps > 0                              # a kept long track's candidate is rejected and formed again
    assert np.isclose(s.final_cost, rs.final_cost, rtol=1e-8)
    assert (s.iterations, s.num_unsuccessful_steps) == (rs.iterations, rs.num_unsuccessful_steps)
    assert ep <= 1e-6 and el <= 1e-5


def test_pipeline_marginalize_sparsify_sparse_priors_solve(backend_cls, oracle_lib):
    w = ph.case_window(ph.CASE["KMIX"])
    args = ph.marg_args(w)
    opts = capi.reference_options()
    po = oracle_lib.marginalize(w, **args)
    fo = oracle_lib.sparsify(w, po, vio=False)
    be = backend(backend_cls)
    try:
        be.set_windows([w])
        same_factors(be.sparsify(0, po, vio=False), fo)              # the same prior: test_gpu_sparsify.py's bar
        pg = be.marginalize(0, **args)
        fg = be.sparsify(0, pg, vio=False)
        assert len(fg) == len(fo) == 6 and {f["type"] for f in fg} == {capi.SPARSE_LMK_PRIOR, capi.SPARSE_LMK_TO_LMK}
        long_ = set(lh.long_landmarks(w).tolist())
        assert any(f["lmk0"] in long_ or f["lmk1"] in long_ for f in fg)
        for a, b in zip(fg, fo):   # the two priors agree to ~1e-8, the information square roots inherit that (test_gpu_sparsify.py)
            assert (a["type"], a["lmk0"], a["lmk1"]) == (b["type"], b["lmk0"], b["lmk1"])
            assert np.abs(a["sqrt_inf"] - b["sqrt_inf"]).max() <= 1e-5 * np.abs(b["sqrt_inf"]).max()
        be.set_windows([ph.sparse_window(w, fg)])
        s = be.solve(opts)[0]
        d = be.get_deltas(0)
    finally:
        be.close()
    ref = oracle_lib.solve(ph.sparse_window(w, fo), opts)
    rs, ep, el = _compare_solve("marginalize -> sparsify -> sparse priors -> solve KMIX", s, d, ref)
    assert s.iterations == rs.iterations
    assert np.isclose(s.final_cost, rs.final_cost, rtol=1e-9)                 # test_gpu_sparse.py's bar
    assert ep <= 1e-6 and el <= 1e-5


_kvio = []


def kvio():
    if not _kvio:
        _kvio.append(ph.kvio())
    return _kvio[0]


def test_kvio_marginalize_keeps_the_long_track_beside_the_kept_frame(backend_cls, oracle_lib):
    """KVIO: the 66-observation landmark is kept beside the kept frame's 15 columns (kf_keep = n_kf - 2, marg_has_imu)."""
    w = kvio()
    args = ph.vio_marg_args(w)
    assert int(lh.long_landmarks(w)[0]) in args["lmk_keep"]
    be = backend(backend_cls)
    try:
        be.set_windows([w])
        pg = be.marginalize(0, **args)
    finally:
        be.close()
    assert pg["kf_col"] == 0 and pg["n"] == 15 + 3 * len(args["lmk_keep"])
    check_prior(pg, oracle_lib.marginalize(w, **args))


def test_kvio_pipeline_marginalize_resident_prior_solve(backend_cls, oracle_lib):
    """KVIO: marginalize -> set_dense_prior(resident) -> solve: the long track is kept by the dense prior beside the kept frame's 15
    columns in a window of 15 states per key-frame, at the bars of test_gpu_marg.py's pipeline test."""
    w = kvio()
    args = ph.vio_marg_args(w)
    opts = capi.reference_options()
    be = backend(backend_cls)
    try:
        be.set_windows([w])
        g = be.marginalize(0, readback=False, **args)
        assert g.get("J") is None
        be.set_windows([ph.next_window(w, g)])
        s = be.solve(opts)[0]
        d = be.get_deltas(0)
    finally:
        be.close()
    o = oracle_lib.marginalize(w, **args)
    ref = oracle_lib.solve(w, opts, dense_prior={k: o[k] for k in ph.PRIOR_KEYS})
    rs, ep, el = _compare_solve("marginalize -> resident prior -> solve KVIO", s, d, ref)
    assert np.isclose(s.final_cost, rs.final_cost, rtol=1e-8)
    assert s.iterations == rs.iterations
    assert ep <= 1e-6 and el <= 1e-5


def test_kvio_sparsified_vio_pipeline(backend_cls, oracle_lib):
    """KVIO: sparsifyVIO puts a pose-to-landmark factor on the kept long track, which holds it in the reduced system of the next solve.
    Every figure is printed before the first assertion. The marginalisation stands on a previous prior on the marginalised frame's
    15 states (long_prior_helpers.vio_marg_args): without one the kept frame's covariance block, which sparsifyVIO inverts, is
    singular. The long track's factor goes into the solve with its information raised 16-fold on both sides
    (long_prior_helpers.raise_long_factor), so that the pose bar sees the factor (tests/test_long_prior_cpu.py). The cost is held at
    test_gpu_sparse.py's 1e-9, poses and landmarks at 1e-6 / 1e-5."""
    w = kvio()
    args = ph.vio_marg_args(w)
    long_ = int(lh.long_landmarks(w)[0])
    opts = capi.reference_options()
    po = oracle_lib.marginalize(w, **args)
    fo = oracle_lib.sparsify(w, po, vio=True)
    be = backend(backend_cls)
    try:
        be.set_windows([w])
        f_same = be.sparsify(0, po, vio=True)
        pg = be.marginalize(0, **args)
        fg = be.sparsify(0, pg, vio=True)
        be.set_windows([ph.sparse_window(w, ph.raise_long_factor(fg, long_))])
        s = be.solve(opts)[0]
        d = be.get_deltas(0)
    finally:
        be.close()
    ref = oracle_lib.solve(ph.sparse_window(w, ph.raise_long_factor(fo, long_)), opts)
    rel = lambda a, b: np.abs(a["sqrt_inf"] - b["sqrt_inf"]).max() / np.abs(b["sqrt_inf"]).max()
    for i, (a, b, c) in enumerate(zip(f_same, fg, fo)):
        print(f"LONGPRIOR KVIO factor {i} type {c['type']} kf {c['kf']} lmk {c['lmk0']}: sqrt_inf against the oracle's: same prior {rel(a, c):.1e} (bar 1e-7), "
              f"device prior {rel(b, c):.1e} (bar 1e-5), max |W| {np.abs(c['sqrt_inf']).max():.1e}")
    rs, ep, el = _compare_solve("marginalize -> sparsify -> sparse priors -> solve KVIO", s, d, ref)
    assert len(fg) == len(fo) and any(f["type"] == capi.SPARSE_POSE_TO_LMK and f["lmk0"] == long_ for f in fg)
    same_factors(f_same, fo)                                          # the same prior: test_gpu_sparsify.py's bar
    for a, b in zip(fg, fo):
        assert rel(a, b) <= 1e-5
    assert s.iterations == rs.iterations
    assert np.isclose(s.final_cost, rs.final_cost, rtol=1e-9)                 # test_gpu_sparse.py's bar
    assert ep <= 1e-6 and el <= 1e-5


@pytest.mark.parametrize("i", [0, 1], ids=["KMIX", "VIO"])
def test_a_pose_to_landmark_factor_holds_a_free_long_track(backend_cls, oracle_lib, i):
    name, w, f = ph.p2l_windows()[i]
    ws = ph.sparse_window(w, [f])
    opts = capi.reference_options()
    be = backend(backend_cls, profile_kernels=True)
    try:
        be.set_windows([ws])
        s = be.solve(opts)[0]
        d, kt = be.get_deltas(0), be.kernel_times()
    finally:
        be.close()
    assert "k_long_lin" in kt and "k_build_kept" in kt, sorted(kt)     # held, not eliminated
    ref = oracle_lib.solve(ws, opts)
    rs, ep, el = _compare_solve(f"pose-to-landmark factor on long track {f['lmk0']} of {name}", s, d, ref)
    assert s.iterations == rs.iterations
    assert np.isclose(s.final_cost, rs.final_cost, rtol=1e-9)
    assert ep <= 1e-6 and el <= 1e-5


# ---- 4. graph and re-plan ------------------------------------------------------------------------------------------------------------------
def test_graph_is_recaptured_when_a_prior_takes_and_releases_long_tracks(backend_cls, oracle_lib):
    """One handle with use_graph = 1: KMIX, KMIX under the prior that keeps three of its long tracks, KMIX again. The sums go through
    global atomics from several workgroups, so each solve equals a fresh handle's to 1e-10 relative (the figure
    test_graph_is_recaptured_when_long_tracks_come_and_go uses for such sums)."""
    case = ph.CASE["KMIX"]
    free, kept = ph.case_window(case), ph.case_prior_window(case, oracle_lib)
    opts = capi.gn_options(4)

    def solve(be, w):
        be.set_windows([w])
        be.solve(opts)
        return be.solve(opts)[0], be.get_deltas(0)                   # the replay of the captured graph

    be = backend(backend_cls, use_graph=True)
    try:
        got = [solve(be, w) for w in (free, kept, free)]
    finally:
        be.close()
    fresh = []
    for w in (free, kept):
        be = backend(backend_cls, use_graph=True)
        try:
            fresh.append(solve(be, w))
        finally:
            be.close()
    rel = lambda a, b: np.abs(a - b).max() / np.abs(b).max()
    for i, j in ((0, 0), (1, 1), (2, 0)):
        ep, el = rel(got[i][1]["pose"], fresh[j][1]["pose"]), rel(got[i][1]["lmk"], fresh[j][1]["lmk"])
        print(f"LONGPRIOR graph: solve {i} against a fresh handle: pose {ep:.1e} lmk {el:.1e} cost {got[i][0].final_cost:.12g} / {fresh[j][0].final_cost:.12g}")
        assert got[i][0].iterations == fresh[j][0].iterations and abs(got[i][0].final_cost - fresh[j][0].final_cost) <= 1e-10 * fresh[j][0].final_cost
        assert ep <= 1e-10 and el <= 1e-10
    assert rel(got[1][1]["lmk"], got[0][1]["lmk"]) > 1e-6            # the prior changed the solve


# ---- 5. the flags ------------------------------------------------------------------------------------------------------------------------------
def test_long_track_priors_without_long_tracks_is_refused_at_create(backend_cls):
    with pytest.raises(capi.SadvioError) as ei:
        backend_cls(device=0, long_track_priors=True)
    msg = str(ei.value)
    print(f"LONGPRIOR create: {msg}")
    assert f"rc={capi.E_INVALID_ARG}:" in msg and "SADVIO_CFG_LONG_TRACK_PRIORS" in msg and "SADVIO_CFG_LONG_TRACKS" in msg


def _prior_calls(be, w, prior, args):
    return {
        "marginalize": lambda: be.marginalize(0, **args),
        "sparsify": lambda: be.sparsify(0, prior, vio=False),
        "set_dense_prior": lambda: be.set_dense_prior(0, prior),
    }


def test_a_handle_with_long_tracks_alone_keeps_its_refusals(backend_cls, oracle_lib):
    case = ph.CASE["KMIX"]
    w = ph.case_window(case)
    prior = ph.case_prior_window(case, oracle_lib).dense_prior
    be = backend_cls(device=0, long_tracks=True)
    try:
        be.set_windows([w])
        for what, call in _prior_calls(be, w, prior, ph.marg_args(w)).items():
            with pytest.raises(capi.SadvioError) as ei:
                call()
            assert f"rc={capi.E_INVALID_ARG}:" in str(ei.value) and lh.LONG_TEXT in str(ei.value), (what, str(ei.value))
        with pytest.raises(capi.SadvioError) as ei:
            be.set_windows([ph.sparse_window(w, oracle_lib.sparsify(w, prior, vio=False))])
        assert lh.LONG_TEXT in str(ei.value)
    finally:
        be.close()


def test_with_both_flags_pseudo_observations_still_must_not_take_a_landmark_past_64(backend_cls):
    """A 63-observation landmark is not a long track: a pose-to-landmark factor on it rides the elimination as two pseudo-observations,
    and 63 + 2 is refused with the text it always had, on a handle with both flags too."""
    import dataclasses
    import test_gpu_tile_packing as tp
    full = ph.case_window(ph.CASE["KL65"])
    w = tp._assemble(full, [(full, l, np.arange(63)) for l in range(full.n_lmk)])
    f = ph.p2l_factor(w, 0, 0)
    be = backend(backend_cls)
    try:
        be.set_windows([w])
        arr, n = dataclasses.replace(w, sparse_priors=[f], _keep=[]).sparse_c()
        rc = be.lib.sadvio_ba_set_sparse_priors(be.h, 0, n, arr)
        msg = be.lib.sadvio_ba_last_error(be.h).decode()
        assert rc == capi.E_INVALID_ARG and lh.LONG_TEXT in msg and "pseudo-observations" in msg, msg
        with pytest.raises(capi.SadvioError) as ei:
            be.set_windows([ph.sparse_window(w, [f])])
        assert lh.LONG_TEXT in str(ei.value)
    finally:
        be.close()


def test_with_both_flags_the_calls_not_served_still_refuse_and_leave_the_state_alone(backend_cls, oracle_lib):
    case = ph.CASE["KMIX"]
    w = ph.case_prior_window(case, oracle_lib)
    be = backend(backend_cls)
    try:
        be.set_windows([w])
        be.solve(capi.gn_options(2))
        before = be.get_deltas(0)
        calls = {
            "covariance": lambda: be.covariance(0, kf=[0]),
            "covariance_batch": lambda: be.covariance_batch([{"w": 0, "kf": [0]}]),
            "covariance_cross": lambda: be.covariance_cross(0, kf=[0], lmk=[5]),
            "marginalize_relative": lambda: be.marginalize_relative(0, 0, 1),
            "marginalize_relative_batch": lambda: be.marginalize_relative_batch(0, [(0, 1)]),
        }
        for what, call in calls.items():
            with pytest.raises(capi.SadvioError) as ei:
                call()
            msg = str(ei.value)
            print(f"LONGPRIOR refusal {what}: {msg}")
            assert f"rc={capi.E_INVALID_ARG}:" in msg and lh.LONG_TEXT in msg, (what, msg)
        after = be.get_deltas(0)
        for k in before:
            assert before[k].tobytes() == after[k].tobytes(), k
    finally:
        be.close()
