"""A layout the planner refuses (layout_plan.h) leaves the handle in a state that says so: no solve on half-built tables, the next valid
window solves to the oracle, and a refused change of the reduced layout leaves the uploaded window as it was. All refusals are host
decisions taken before anything is queued for the device. Window: 3 key-frames, 6 landmarks, 2 cameras; solves are held to the bars
of test_gpu_tile_packing._check_against_oracle (final cost rtol 1e-9, the reference's step counts, steps to 1e-6)."""
import dataclasses

import numpy as np
import pytest

from golden_util import lmk_err
from sadvio_amd import capi, synthetic
from test_gpu_parity import LMK_TOL, POSE_TOL

pytestmark = pytest.mark.gpu

TOO_MANY = "set_windows: a landmark has more than 64 observations"


def _window(seed=21):
    return synthetic.make_window(n_kf=3, n_lmk=6, seed=seed)


def _with_65_observations(w):
    """w with the first landmark's first observation repeated until the landmark has 65."""
    extra = 65 - int(w.lmk_obs_ptr[1])
    ptr = w.lmk_obs_ptr.copy(); ptr[1:] += extra
    rep = lambda a: np.concatenate([np.repeat(a[:1], extra, axis=0), a])
    return dataclasses.replace(w, lmk_obs_ptr=ptr.astype(np.int32), obs_kf=rep(w.obs_kf), obs_cam=rep(w.obs_cam), obs_meas=rep(w.obs_meas))


def _solves_to_oracle(be, oracle_lib, w):
    opts = capi.reference_options()
    s = be.solve(opts)[0]
    d = be.get_deltas(0)
    ref = oracle_lib.solve(w, opts)
    rs = ref["summary"]
    assert np.isclose(s.final_cost, rs.final_cost, rtol=1e-9)
    assert (s.iterations, s.termination) == (rs.iterations, rs.termination)
    assert (s.num_successful_steps, s.num_unsuccessful_steps) == (rs.num_successful_steps, rs.num_unsuccessful_steps)
    assert np.abs(d["pose"] - ref["pose"]).max() <= POSE_TOL and lmk_err(d["lmk"], ref["lmk"]) <= LMK_TOL


@pytest.mark.parametrize("one_build", [False, True])   # True: inside begin_update .. commit_update, the refusal arrives at commit
def test_refused_window_is_not_solved_and_the_next_one_is(backend_cls, oracle_lib, one_build):
    w = _window()
    be = backend_cls(device=0)
    try:
        be.set_windows([w], one_build=one_build)     # a layout is on the device when the refusal comes
        with pytest.raises(capi.SadvioError) as e:
            be.set_windows([_with_65_observations(w)], one_build=one_build)
        assert f"rc={capi.E_INVALID_ARG}:" in str(e.value) and TOO_MANY in str(e.value)
        with pytest.raises(capi.SadvioError) as e:
            be.solve(capi.reference_options())
        assert f"rc={capi.E_STATE}:" in str(e.value)
        be.set_windows([w], one_build=one_build)
        _solves_to_oracle(be, oracle_lib, w)
    finally:
        be.close()


def test_refused_resident_prior_leaves_the_uploaded_windows_solvable(backend_cls):
    ws = [_window(21), _window(22)]
    J0 = np.diag(np.concatenate([10.0 * np.ones(6), 5.0 * np.ones(3), 20.0 * np.ones(3), 50.0 * np.ones(3)]))
    attach = {"resident": True, "kf_keep": 1, "kf_col": 0}
    opts = capi.reference_options()
    be = backend_cls(device=0)
    try:
        be.set_prior(J0, np.zeros(15))
        be.set_windows(ws)
        be.set_dense_prior(0, attach)
        before = [(s.final_cost, s.iterations, s.termination) for s in be.solve(opts)]
        be.set_prior(2.0 * J0, np.zeros(15))         # window 0 attached the prior that this replaces
        with pytest.raises(capi.SadvioError) as e:
            be.set_dense_prior(1, attach)
        assert f"rc={capi.E_STATE}:" in str(e.value) and "attach it again" in str(e.value)
        after = [(s.final_cost, s.iterations, s.termination) for s in be.solve(opts)]
        for a, b in zip(after, before):
            assert a[1:] == b[1:] and np.isclose(a[0], b[0], rtol=1e-9)
    finally:
        be.close()


def test_refused_rebuild_inside_a_factor_setter_leaves_no_layout(backend_cls, oracle_lib):
    """With sparse priors on the window, set_dense_prior rebuilds the whole layout (which factors are eliminable may change). When that
    rebuild is refused, the host tables are half replaced over the old device data: the handle must say it has no layout."""
    from sparse_helpers import vo_sparse_priors
    ws = [_window(21), _window(22)]
    ws[1].sparse_priors = vo_sparse_priors(ws[1], [0, 2, 4], np.random.default_rng(5))
    J0 = np.diag(np.concatenate([10.0 * np.ones(6), 5.0 * np.ones(3), 20.0 * np.ones(3), 50.0 * np.ones(3)]))
    attach = {"resident": True, "kf_keep": 1, "kf_col": 0}
    be = backend_cls(device=0)
    try:
        be.set_prior(J0, np.zeros(15))
        be.set_windows(ws)
        be.set_dense_prior(0, attach)
        be.solve(capi.reference_options())
        be.set_prior(2.0 * J0, np.zeros(15))
        with pytest.raises(capi.SadvioError) as e:
            be.set_dense_prior(1, attach)            # window 1 carries sparse priors: a full rebuild, refused for window 0's stale prior
        assert f"rc={capi.E_STATE}:" in str(e.value) and "attach it again" in str(e.value)
        with pytest.raises(capi.SadvioError) as e:
            be.solve(capi.reference_options())
        assert f"rc={capi.E_STATE}:" in str(e.value)
        w = _window(21)
        be.set_windows([w])                          # and the handle takes the next window
        _solves_to_oracle(be, oracle_lib, w)
    finally:
        be.close()
