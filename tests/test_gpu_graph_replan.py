"""The captured graph of a solve is keyed on the solve's plan (solve_driver.h: the bytes of SolvePlan and of every window's BigPlan).
One handle with use_graph=True goes through a sequence of (window, options) steps, consecutive steps differing in one plan field;
every step solves twice, so its second solve replays the graph its first one captured. A plan field missing from the key would
replay the graph of the step before: every solve is held against a fresh handle without a graph, and against the oracle."""
import numpy as np
import pytest

from sadvio_amd import capi, synthetic
from test_gpu_edges import agree
from vio_helpers import make_vio_window

pytestmark = pytest.mark.gpu

# device against device (tests/test_gpu_edges.py, handle reuse): only the order of the tiles' atomics differs
POSE_DEV_TOL = 1e-11
LMK_DEV_TOL = 1e-9


def _huber(opts):
    opts.huber_a = 1.345 ** 0.5
    return opts


def _steps():
    small = synthetic.make_window(n_kf=6, n_lmk=300, seed=17)
    more_tiles = synthetic.make_window(n_kf=8, n_lmk=900, seed=77)
    vio = make_vio_window(n_kf=6, n_lmk=300, seed=5)
    # Out of LDS (N_p = 210, then 282): the test pins that much, by k_solve_front among the kernel classes. Which of the out-of-LDS
    # routes the two windows take (band = 5 is meant to give a band route, whose workspace d_big_linv = 6 N_p doubles then grows and
    # moves at the larger window) is not pinned, and the larger window's plan differs in N_p as well: no step isolates a workspace
    # pointer as the only key field that changed.
    big = synthetic.make_window(n_kf=36, n_lmk=2500, length=18.0, band=5, seed=22)
    bigger = synthetic.make_window(n_kf=48, n_lmk=1500, length=24.0, band=5, seed=23)
    # (name, window, options, VIO window, out of LDS): what changes against the step before
    return [
        ("start", small, capi.gn_options(6), False, False),
        ("slots", small, capi.gn_options(3), False, False),
        ("tiles_mtk", more_tiles, capi.gn_options(3), False, False),
        ("extras_imu_pf", vio, capi.gn_options(3), True, False),
        ("rare", vio, _huber(capi.gn_options(3)), True, False),
        ("out_of_lds", big, capi.gn_options(3), False, True),
        ("out_of_lds_larger", bigger, capi.gn_options(3), False, True),
        ("out_of_lds", big, capi.gn_options(3), False, True),
        ("start", small, capi.gn_options(6), False, False),
    ]


def _close(d, e):
    return np.abs(d["pose"] - e["pose"]).max() <= POSE_DEV_TOL and np.abs(d["lmk"] - e["lmk"]).max() <= LMK_DEV_TOL


def test_graph_follows_the_plan_through_a_sequence_of_solves(backend_cls, oracle_lib):
    refs = {}   # per distinct step: the oracle's solve, a fresh graph-less handle's solve and the kernel classes it launched
    first = {}  # the graph handle's first result of a step that comes back later in the sequence
    be = backend_cls(device=0, use_graph=True)
    try:
        for name, w, opts, is_vio, out_of_lds in _steps():
            if name not in refs:
                fresh = backend_cls(device=0, use_graph=False, profile_kernels=True)
                try:
                    fresh.set_windows([w])
                    fs = fresh.solve(opts)[0]
                    refs[name] = (oracle_lib.solve(w, opts), fs, fresh.get_deltas(0), set(fresh.kernel_times()))
                finally:
                    fresh.close()
                names = refs[name][3]
                assert ("k_solve_front" in names) == out_of_lds, (name, names)          # the route the step is here for
                assert ("k_solve" in names) == (not out_of_lds), (name, names)
                if is_vio:
                    assert "k_pf_lin" not in names, (name, names)                        # the IMU pairs ride k_build (with_imu)
            ref, fs, fd, _ = refs[name]
            be.set_windows([w])
            for attempt in ("capture", "replay"):
                s = be.solve(opts)[0]
                d = be.get_deltas(0)
                assert (s.iterations, s.termination) == (fs.iterations, fs.termination), (name, attempt)
                assert _close(d, fd), (name, attempt, np.abs(d["pose"] - fd["pose"]).max(), np.abs(d["lmk"] - fd["lmk"]).max())
                agree(be, 0, w, ref, s, vio=is_vio)
                if name in first:
                    assert _close(d, first[name]), (name, attempt, "differs from the same step earlier in the sequence")
            first.setdefault(name, d)
    finally:
        be.close()
