"""CPU checks behind tests/test_gpu_long_priors.py (no GPU):
  - the E_REF table of tests/long_prior_helpers.py brackets the oracle's measured float64 error against the 50-digit step on every
    window under its prior, the oracle accepts that step, and its trace row carries the 50-digit model cost change and cost;
  - the committed 50-digit fixture equals a fresh computation (on the cheapest window);
  - the windows and priors are what their names say;
  - the bars see the defects a kept long track can have on the device, each planted in the un-reduced system of the oracle and solved
    in 50 digits; each lands more than 1e3 x above the bar of the GPU test:
      (a) the kept long track's step left at zero by the back-substitution (k_long_back without its lcode == 2 branch);
      (b) one of its 65 observations missing from the kept list (k_build_kept adds the landmark's rows from that list, k_long_lin the
          pose-pose part from the landmark's own observations: the landmark's rows and columns and its gradient lose the observation,
          the pose-pose block keeps it);
      (c) its pose-pose part counted twice (k_long_lin and a tile both summing it)."""
import numpy as np
import pytest

import long_prior_helpers as ph
import long_track_helpers as lh
import step_helpers as sh

mp = pytest.importorskip("mpmath")


@pytest.mark.parametrize("case", ph.CASES, ids=[c.name for c in ph.CASES])
def test_e_ref_table_brackets_the_measured_values(oracle_lib, case):
    w = ph.case_prior_window(case, oracle_lib)
    f64 = sh.oracle_step(oracle_lib, w, ph.case_options(case))
    ref = ph.reference(case)
    e = sh.step_error(f64, ref, w)
    print(f'E_REF "{case.window}": ({e[0]:.2e}, {e[1]:.2e}),')
    for part, m, t in zip(("pose", "landmark"), e, ph.E_REF[case.window]):
        assert m <= t <= 4.0 * m, (part, m, t)
    assert np.isclose(f64["log"][1][7], ref["model_cost_change"], rtol=1e-11)
    assert np.isclose(f64["log"][1][0], ref["cost"], rtol=1e-11)


def test_fixture_equals_a_fresh_50_digit_step(oracle_lib):
    case = ph.CASE["KL65_angular"]
    fresh, stored = ph.reference(case, oracle_lib, fresh=True), ph.reference(case)
    for k in ("pose", "lmk", "dv", "dba", "dbg"):
        assert np.array_equal(fresh[k], stored[k]), k
    assert fresh["model_cost_change"] == stored["model_cost_change"] and fresh["cost"] == stored["cost"]


def test_windows_and_priors_are_what_their_names_say(oracle_lib):
    kl, km = ph.case_window(ph.CASE["KL65"]), ph.case_window(ph.CASE["KMIX"])
    assert set(lh.counts(kl)) == {65} and kl.n_kf == 34 and kl.kf_const.sum() == 29
    kf0 = kl.n_kf - 1
    seen = [l for l in range(kl.n_lmk) if (kl.obs_kf[kl.lmk_obs_ptr[l]:kl.lmk_obs_ptr[l + 1]] == kf0).any()]
    assert len(seen) == 8
    a = ph.marg_args(kl)
    assert len(a["lmk_keep"]) == 5 and a["lmk_marg"] == []
    n = lh.counts(km)
    assert km.n_kf == 34 and km.kf_const.sum() == 28 and (n == 5).sum() == 120 and (n == 66).sum() == 4
    assert lh.long_landmarks(km).tolist() == [0, 61, 62, 123]
    a = ph.marg_args(km)
    long_ = set(lh.long_landmarks(km).tolist())
    assert len(a["lmk_keep"]) == 6 and len(set(a["lmk_keep"]) & long_) == 3 and a["lmk_marg"] == []
    for case in ph.CASES:                                            # the prior of every case keeps what the table says, in N_p = poses + 3 per kept landmark
        w = ph.case_prior_window(case, oracle_lib)
        lay = sh.layout(w)
        assert lay["Nr"] == lay["dpf"] * int((np.asarray(w.kf_const) == 0).sum()) + 3 * case.n_keep
        assert (lay["Nr"] > sh.MAX_LDS_NP) == (case.name == "KBIG")                      # KBIG alone is solved out of LDS
    assert sh.layout(ph.case_prior_window(ph.CASE["KVIO"], oracle_lib))["dpf"] == 15
    assert sh.reduced_np(ph.case_prior_window(ph.CASE["KBIG"], oracle_lib)) == 249 and set(lh.counts(ph.case_window(ph.CASE["K258"]))) == {258}
    share = sh.beyond_huber(ph.case_window(ph.CASE["KL65_huber"]))
    assert 0.1 <= share <= 0.9, share


def test_the_pose_to_landmark_factor_on_a_long_track_moves_the_solution(oracle_lib):
    """The bars of test_a_pose_to_landmark_factor_holds_a_free_long_track (pose 1e-6, landmark 1e-5) see a dropped factor: without it
    the oracle's solution moves by more than 10 x those bars."""
    from sadvio_amd import capi
    opts = capi.reference_options()
    for name, w, f in ph.p2l_windows():
        assert f["lmk0"] in lh.long_landmarks(w) and w.kf_const[f["kf"]] == 0
        with_f, without = oracle_lib.solve(ph.sparse_window(w, [f]), opts), oracle_lib.solve(w, opts)
        ep, el = np.abs(with_f["pose"] - without["pose"]).max(), np.abs(with_f["lmk"] - without["lmk"]).max()
        print(f"{name}: without its pose-to-landmark factor the solution moves by pose {ep:.1e} landmark {el:.1e}")
        assert ep > 10 * 1e-6 and el > 10 * 1e-5


def test_kvio_has_a_prior_that_sparsify_vio_can_invert(oracle_lib):
    """KVIO's marginalisation stands on a previous prior on the marginalised frame's 15 states: the prior then has full rank and the kept
    frame's covariance block, which sparsifyVIO's IMU prior factor inverts, is well conditioned. Without the previous prior that block
    is singular, and the factor compared by test_kvio_sparsified_vio_pipeline would not be a defined quantity. The factor that
    sparsifyVIO puts on the long track: the kept frame is constant in this shape, and as sparsified the factor, dropped, moves the
    oracle's poses by 7.5e-6, less than 10 x the pose bar (1e-6). So the pipeline test solves with the factor's information raised
    16-fold (long_prior_helpers.raise_long_factor, square-root information x 4), as the issue provides for: dropped then, the oracle's
    solution moves by more than 10 x the pose bar and 10 x the landmark bar of the GPU test."""
    from sadvio_amd import capi
    w = ph.kvio()
    args = ph.vio_marg_args(w)
    long_ = int(lh.long_landmarks(w)[0])
    assert w.has_imu == 1 and w.n_kf == 36 and int((w.kf_const == 0).sum()) == 6 and lh.counts(w)[long_] == 66 and long_ in args["lmk_keep"]
    po = oracle_lib.marginalize(w, **args)
    rank, n, cond = ph.kept_frame_covariance_cond(po)
    bare = oracle_lib.marginalize(w, **{k: v for k, v in args.items() if k != "last"})
    rank0, n0, cond0 = ph.kept_frame_covariance_cond(bare)
    print(f"KVIO prior: rank {rank} of {n}, cond of the kept frame's covariance block {cond:.1e}; without the previous prior rank {rank0} of {n0}, cond {cond0:.1e}")
    assert rank == n == po["n_full"] == 15 + 3 * len(args["lmk_keep"]) and cond < 1e4
    assert rank0 < n0 and cond0 > 1e12
    fo = oracle_lib.sparsify(w, po, vio=True)
    on_long = [f for f in fo if f["type"] == capi.SPARSE_POSE_TO_LMK and f["lmk0"] == long_]
    assert len(on_long) == 1
    opts = capi.reference_options()
    dropped = oracle_lib.solve(ph.sparse_window(w, [f for f in fo if f is not on_long[0]]), opts)
    for k in (1.0, ph.LONG_FACTOR_RAISE):
        full = oracle_lib.solve(ph.sparse_window(w, ph.raise_long_factor(fo, long_, k)), opts)
        ep, el = np.abs(full["pose"] - dropped["pose"]).max(), np.abs(full["lmk"] - dropped["lmk"]).max()
        print(f"KVIO without the long track's pose-to-landmark factor (square-root information x {k:g}): pose {ep:.1e} landmark {el:.1e}")
    assert ep > 10 * 1e-6 and el > 10 * 1e-5


# ---- the defects ---------------------------------------------------------------------------------------------------------------------------
def _kept_long(w):
    return [int(l) for l, c in zip(w.dense_prior["lmk_index"], w.dense_prior["lmk_col"]) if c >= 0 and l in lh.long_landmarks(w)]


def _without_observation(w, l, pos):
    """w with the observation at position pos of landmark l removed (the prior and the ids kept)."""
    import dataclasses
    import test_gpu_tile_packing as tp
    keep = np.setdiff1d(np.arange(lh.counts(w)[l]), [pos])
    d = tp._assemble(w, [(w, q, keep if q == l else None) for q in range(w.n_lmk)])
    return dataclasses.replace(d, kf_id=w.kf_id, lmk_id=w.lmk_id, dense_prior=w.dense_prior, _keep=[])


def _report(what, case, e):
    bar_p, bar_l = ph.bars(case)
    print(f"{case.name} {what}: pose {e[0]:.1e} ({e[0] / bar_p:.1e} x bar) landmark {e[1]:.1e} ({e[1] / bar_l:.1e} x bar)")
    assert e[0] > 1e3 * bar_p or e[1] > 1e3 * bar_l


def test_a_kept_long_track_whose_step_stays_zero_lands_far_above_the_bar(oracle_lib):
    case = ph.CASE["KL65"]
    w = ph.case_prior_window(case, oracle_lib)
    got = sh.oracle_step(oracle_lib, w, ph.case_options(case))
    got = dict(got, lmk=got["lmk"].copy())
    got["lmk"][_kept_long(w)[0]] = 0.0                               # what delta_l = -M^-1 t gives with M^-1 = 0
    _report("kept long track left where it was", case, sh.step_error(got, ph.reference(case), w))


def _pose_cols(w, l, pos):
    """Columns of the free key-frame that observes landmark l at position pos (None: a constant key-frame)."""
    k = int(w.obs_kf[w.lmk_obs_ptr[l] + pos])
    off = sh.layout(w)["kf_off"][k]
    return None if off < 0 else np.arange(off, off + 6)


def test_an_observation_missing_from_the_kept_list_lands_far_above_the_bar(oracle_lib):
    case = ph.CASE["KL65"]
    w = ph.case_prior_window(case, oracle_lib)
    opts = ph.case_options(case)
    l = _kept_long(w)[0]
    pos = next(p for p in range(65) if _pose_cols(w, l, p) is not None)       # an observation from a free key-frame
    H, g = sh.oracle_system(oracle_lib, w, opts)
    Hd, gd = sh.oracle_system(oracle_lib, _without_observation(w, l, pos), opts)
    assert H.shape == Hd.shape
    lc = sh.layout(w)["lmk_red"][l] + np.arange(3)
    Hx, gx = H.copy(), g.copy()
    Hx[lc, :] = Hd[lc, :]; Hx[:, lc] = Hd[:, lc]; gx[lc] = gd[lc]             # the landmark's rows, columns and gradient without it; the pose-pose block with it
    assert np.abs(Hx - H).max() > 0 and np.array_equal(Hx, Hx.T)
    got = sh.mp_first_step(w, opts, system=(Hx, gx), want_cost=False)
    _report("one observation missing from the kept list", case, sh.step_error(got, ph.reference(case), w))


def test_a_pose_pose_part_counted_twice_lands_far_above_the_bar(oracle_lib):
    case = ph.CASE["KL65"]
    w = ph.case_prior_window(case, oracle_lib)
    opts = ph.case_options(case)
    l = _kept_long(w)[0]
    H, g = sh.oracle_system(oracle_lib, w, opts)
    Hx, gx = H.copy(), g.copy()
    n_pose = 6 * int((np.asarray(w.kf_const) == 0).sum())
    for pos in range(65):                                            # what each observation adds to the pose-pose block and the pose gradient: by difference
        pc = _pose_cols(w, l, pos)
        if pc is None:
            continue
        Hd, gd = sh.oracle_system(oracle_lib, _without_observation(w, l, pos), opts)
        Hx[np.ix_(pc, pc)] += (H - Hd)[np.ix_(pc, pc)]; gx[pc] += (g - gd)[pc]
    assert np.abs((Hx - H)[:n_pose, :n_pose]).max() > 0 and np.array_equal((Hx - H)[n_pose:], np.zeros_like(H[n_pose:]))
    got = sh.mp_first_step(w, opts, system=(Hx, gx), want_cost=False)
    _report("pose-pose part of a kept long track counted twice", case, sh.step_error(got, ph.reference(case), w))
