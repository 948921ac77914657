"""The first LM step of every reduced-solve route and of every tile-kernel variant against the 50-digit step (tests/step_helpers.py).

One solve of ONE iteration per case: k_solve<0, false> (VO, N_p = 6 .. 174 at every size where chol16.h's c16_solve branches),
k_solve<0, true> (VIO and kept landmarks), and the five out-of-LDS routes of solve_driver.h at their boundary sizes. The step must lie
within TOL_FACTOR x max(E_REF, FLOOR) of the 50-digit one, where E_REF is the float64 oracle's own distance from it
(tests/test_step_reference_cpu.py keeps that table honest and proves that this bar sees a single unrefined reciprocal square root, a
dropped rank-4 product and a missing damping term); the trace row of the step must carry the 50-digit model cost change and cost to
1e-11. The whole-solve tests hold the same code to 1e-6 only.

The tile kernels carry most of the arithmetic of a step, and the cases above reach k_solve through one tile path only (packed
single-round MFMA tiles of k_build, then k_backsub). step_helpers.TILE_CASES hold their other variants to the same bar on small
windows: the contiguous cut, no first-round packets, two and three landmark rounds per tile, constant key-frames and landmarks,
k_build<RARE> / k_backsub<RARE> under Huber, 16 / 32 / 64 lanes per landmark and a 6-free-key-frame tile (lds_mode 1), the IMU pairs
outside the tile workgroups, and the throughput kernels k_lm_pass0 / k_build_obs / k_lm_pass (SADVIO_LM=1) at every chunk cut, at one
and five free key-frames, with two sub-blocks per tile and at window index 2 of a batch. Each of them asserts from kernel_times()
which kernels ran; tests/test_tile_plan_cpu.py asserts on the host that the planner gave each window the tiles it is meant to have.

Every case prints its measured multiples (`FIRST_STEP ...`, run with -s) before it asserts; DESIGN.md section 2 records them."""
import numpy as np
import pytest

import step_helpers as sh
from sadvio_amd import capi

pytestmark = pytest.mark.gpu

SWITCHES = sh.SWITCHES
_device = {}      # case name -> deltas of the device's step (the route-against-route test reuses them)


def run_case(backend_cls, monkeypatch, case, front=None):
    """(summary, deltas, trace, kernel_times) of one iteration on the case's window, stored behind the windows `front` of one batch
    (default: the case's decoys). The switches are set before the handle is created: it reads them once, in create. A case that
    names its kernels runs on a profiling handle, and kernel_times() says which kernels ran."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    ws = sh.case_windows(case) if front is None else list(front) + [sh.case_window(case)]
    i = len(ws) - 1
    be = backend_cls(device=0, profile_kernels=bool(case.kernels))
    try:
        be.set_windows(ws)
        s = be.solve(sh.case_options(case))[i]
        d = be.get_deltas(i)
        tr = be.get_trace(i)
        kt = be.kernel_times() if case.kernels else {}
    finally:
        be.close()
    return s, d, tr, kt


def check_kernels(case, kt):
    """The kernels the case is about are the ones that ran."""
    n = {k: v["launches"] for k, v in kt.items()}
    if case.kernels == "throughput":
        assert (n.get("k_lm_pass0"), n.get("k_build_obs"), n.get("k_lm_pass")) == (1, 1, 1) and "k_build" not in n, n
    elif case.kernels in ("latency", "pf"):
        assert n.get("k_build") == 1 and n.get("k_backsub") == 1 and "k_lm_pass" not in n and "k_build_obs" not in n, n
        assert ("k_pf_lin" in n and "k_pf_cost" in n) == (case.kernels == "pf"), n


def check_case(case, oracle_lib, s, d, tr, n_win=1, tag=""):
    w = sh.case_window(case)
    lay = sh.layout(w)
    assert lay["Nr"] == case.np_
    assert sh.free_kf_observations(w).min() >= 10
    route = sh.expected_route(lay["Nr"], lay["dpf"], sh.band_rows(w), n_win, int(case.env.get("SADVIO_BAND_C", 0)),
                              case.env.get("SADVIO_NO_BCR") == "1")
    assert route == ("lds" if case.route.startswith("lds") else case.route), route
    if route in ("band", "band_twisted", "bcr"):
        assert sh.band_rows(w) == 3 * lay["dpf"] == (sh.half_bandwidth(w) + 1) * lay["dpf"]     # band = 1: three key-frames
    ref = sh.reference(case, oracle_lib)
    e = sh.step_error(d, ref, w)
    unit = [max(v, sh.FLOOR) for v in sh.E_REF[case.window]]
    mcc_rel = abs(tr[1][7] / ref["model_cost_change"] - 1) if len(tr) > 1 else np.inf
    cost_rel = abs(tr[1][0] / ref["cost"] - 1) if len(tr) > 1 else np.inf
    print(f"FIRST_STEP {case.name}{tag} Np {case.np_} {case.route} e_ref {sh.E_REF[case.window][0]:.1e} {sh.E_REF[case.window][1]:.1e} "
          f"multiple pose {e[0] / unit[0]:.2f} lmk {e[1] / unit[1]:.2f} mcc {mcc_rel:.1e} cost {cost_rel:.1e} steps {s.num_successful_steps}")
    assert s.num_successful_steps == 1          # the oracle accepts this step (test_step_reference_cpu.py): a rejection is a failure
    bar_p, bar_l = sh.bars(case)
    assert e[0] <= bar_p, ("pose part", e[0], bar_p)
    assert e[1] <= bar_l, ("landmark part", e[1], bar_l)
    assert np.isclose(tr[1][7], ref["model_cost_change"], rtol=1e-11, atol=0)
    assert np.isclose(tr[1][0], ref["cost"], rtol=1e-11, atol=0)


@pytest.mark.parametrize("case", sh.CASES, ids=[c.name for c in sh.CASES])
def test_first_step_against_50_digits(backend_cls, oracle_lib, monkeypatch, case):
    s, d, tr, kt = run_case(backend_cls, monkeypatch, case)
    _device[case.name] = d
    check_kernels(case, kt)
    check_case(case, oracle_lib, s, d, tr, n_win=len(case.front) + 1)


def test_first_step_at_window_index_2_of_a_batch(backend_cls, oracle_lib, monkeypatch):
    """k_solve runs one workgroup per window: the N_p = 114 window behind two decoys, at the same bar."""
    import batch_helpers as bh
    case = sh.CASE[sh.BATCH_CASE]
    s, d, tr, _ = run_case(backend_cls, monkeypatch, case, front=(bh.decoy(sh.PIXEL, "a"), bh.decoy(sh.PIXEL, "b")))
    check_case(case, oracle_lib, s, d, tr, n_win=3, tag="@2")


@pytest.mark.parametrize("n", [384, 402, 582])
def test_bcr_and_the_band_solver_agree(backend_cls, oracle_lib, monkeypatch, n):
    """The same window through block cyclic reduction and, with SADVIO_NO_BCR=1, through the sliding band solver: within
    TOL_FACTOR x E_REF of each other (each is held to that bar against the 50-digit step by the test above)."""
    a, b = sh.CASE[f"bcr{n}"], sh.CASE[f"nobcr{n}"]
    w = sh.case_window(a)
    da = _device.get(a.name) or run_case(backend_cls, monkeypatch, a)[1]
    db = _device.get(b.name) or run_case(backend_cls, monkeypatch, b)[1]
    ref = sh.reference(a, oracle_lib)
    bar_p, bar_l = sh.bars(a)
    ep = np.abs(sh.pose_part(da, w) - sh.pose_part(db, w)).max() / np.abs(sh.pose_part(ref, w)).max()
    el = np.abs(da["lmk"] - db["lmk"]).max() / np.abs(ref["lmk"]).max()
    print(f"FIRST_STEP bcr{n} against nobcr{n}: pose {ep / bar_p * sh.TOL_FACTOR:.2f} lmk {el / bar_l * sh.TOL_FACTOR:.2f}")
    assert ep <= bar_p and el <= bar_l
