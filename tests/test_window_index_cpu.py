"""The decoys of tests/batch_helpers.py can make a GPU test fail: for every (windows in front, target) pair that
tests/test_gpu_window_index.py uses, a forgotten (or off-by-one-window) kf_base / cam_base / lmk_base / obs_base is emulated on the
host (batch_helpers.global_view) and the oracle's linearisation of the aliased window is compared with that of the true one.

Bar: the GPU tests hold residuals and Jacobians to 1e-10 relative (tests/test_gpu_parity.py); an aliased window must be at least
1e3 x that away (relative, max norm) in the residuals, the pose Jacobians AND the landmark Jacobians, so that no comparison a GPU
test makes could pass by accident. A pair that misses this gets another decoy, not another threshold."""
import numpy as np
import pytest

import batch_helpers as bh

PARITY_BAR = 1e-10          # tests/test_gpu_parity.py
MIN_DISTANCE = 1e3 * PARITY_BAR


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.fixture(scope="module")
def pairs():
    return bh.pairs_used()


def test_decoys_differ_in_every_size(pairs):
    for name, front, target in pairs:
        for d in front:
            if d.n_cam != 3:
                continue     # another target of the same batch (the covariance batch): it differs as a whole window, checked below
            assert d.n_kf != target.n_kf and d.n_lmk != target.n_lmk and d.n_obs != target.n_obs, name
            assert set(np.diff(d.lmk_obs_ptr)) != set(np.diff(target.lmk_obs_ptr)), name
            assert (d.factor_type, d.has_imu) == (target.factor_type, target.has_imu), name
            assert len(set(d.cam_sigma)) == 3 and (d.obs_cam == 0).sum() >= 3, name
            assert np.allclose(d.cam_K[0, :2], 1.05 * d.cam_K[1, :2]) and not np.allclose(d.cam_T_s_f[0], d.cam_T_s_f[1]), name
        assert front[0].n_cam == 3, name          # whatever else is in front, index 0 holds a decoy with three cameras


def test_the_global_view_is_the_target(oracle_lib, pairs):
    """The emulation itself: with every base in place the view linearises bit for bit as the target alone."""
    for name, front, target in pairs:
        a = oracle_lib.linearize(bh.global_view(front, target))
        b = oracle_lib.linearize(target)
        for x, y in zip(a, b):
            assert np.array_equal(x, y), name


def test_every_forgotten_base_moves_the_linearisation(oracle_lib, pairs):
    worst = np.inf
    for name, front, target in pairs:
        r0, Jp0, Jl0, _ = oracle_lib.linearize(target)
        for drop in ("kf", "cam", "lmk", "obs"):
            for wrong in sorted({0, len(front) - 1}):
                if drop == "cam" and front[wrong].n_cam == 2:
                    continue     # the covariance batch (set by its test plan) stores three windows of the same rig side by side:
                                 # taking the neighbour's cam_base reads equal rows; forgetting cam_base altogether is still exposed
                r, Jp, Jl, _ = oracle_lib.linearize(bh.global_view(front, target, drop=drop, wrong=wrong))
                e = (relerr(r, r0), relerr(Jp, Jp0), relerr(Jl, Jl0))
                print(f"[window index] {name}: {drop}_base -> base of window {wrong}: relative distance r {e[0]:.2e} Jp {e[1]:.2e} Jl {e[2]:.2e}")
                worst = min(worst, *e)
                assert min(e) >= MIN_DISTANCE, (name, drop, wrong, e)
    print(f"[window index] smallest distance of an aliased window {worst:.2e}; required {MIN_DISTANCE:.0e}")
