"""GPU parity of solves with a dense prior on both sides of DP_LDS_N = 2 048 (kernels.h: k_prior_r / k_prior_m stage the step of at
most DP_LDS_N prior variables in LDS; a larger prior gathers kind -> index -> delta per row), against live oracle solves with their
iterate-by-iterate trace. The reduced systems have N_p ~ 2 100: the wide-panel dense route."""
import numpy as np
import pytest

from marg_boundary import thresholds
from sadvio_amd import capi, synthetic
from test_gpu_prior import check_solve, compare, random_prior
from vio_helpers import make_vio_window

pytestmark = pytest.mark.gpu

N_THREADS = 16   # the oracle's OpenMP threads: the CPU share of one GPU job


def _vio_case(n_keep, seed):
    w = make_vio_window(n_kf=6, n_lmk=900, seed=seed)
    w.dense_prior = random_prior(w, n_keep, w.n_kf - 2, np.random.default_rng(seed), rank_deficit=2)
    return w


@pytest.mark.parametrize("n_keep", [677, 678])
def test_vio_prior_across_dp_lds_n(backend_cls, oracle_lib, n_keep):
    """VIO, kf_keep: n = 15 + 3 n_keep = 2 046 (staged in LDS) / 2 049 (> DP_LDS_N: gathered per row, a tail of 1 past the
    256-wide loop)."""
    w = _vio_case(n_keep, 700 + n_keep)
    n = w.dense_prior["J"].shape[1]
    assert n == 15 + 3 * n_keep and (n <= thresholds()["DP_LDS_N"]) == (n_keep == 677)
    compare(backend_cls, oracle_lib, w, capi.reference_options(), vio=True, n_threads=N_THREADS)


def test_vo_prior_past_dp_lds_n(backend_cls, oracle_lib):
    """VO, no kept key-frame: n = 3 * 683 = 2 049 > DP_LDS_N."""
    w = synthetic.make_window(n_kf=5, n_lmk=900, seed=783)
    w.dense_prior = random_prior(w, 683, -1, np.random.default_rng(783), rank_deficit=2)
    assert w.dense_prior["J"].shape[1] == 2049 > thresholds()["DP_LDS_N"]
    compare(backend_cls, oracle_lib, w, capi.reference_options(), n_threads=N_THREADS)


def test_batch_with_priors_on_both_sides_of_dp_lds_n(backend_cls, oracle_lib):
    """Two windows in one set_windows, n = 2 046 and 2 049: one launch of k_prior_r / k_prior_m with grid.x = the batch maximum covers
    blocks past the smaller window's rows and makes the staged / per-row choice per window. Each window against its own oracle solve."""
    ws = [_vio_case(677, 801), _vio_case(678, 802)]
    opts = capi.reference_options()
    be = backend_cls(device=0)
    try:
        be.set_windows(ws)
        sums = be.solve(opts)
        got = [(sums[i], be.get_deltas(i), be.get_trace(i)) for i in range(2)]
    finally:
        be.close()
    for w, (s, d, trace) in zip(ws, got):
        check_solve(s, d, trace, oracle_lib.solve(w, opts, dense_prior=w.dense_prior, n_threads=N_THREADS), vio=True)
