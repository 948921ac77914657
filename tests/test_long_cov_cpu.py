"""CPU side of the covariances of windows with long tracks: the float64 yardstick of tests/test_gpu_long_cov.py, planted defects that
its bar must see, and the flag's bindings. No GPU.

e_ref per window = max over two float64 routes of the largest relative block difference (every key-frame block, the far cross pair,
every landmark block) from the 50-digit blocks of cov_helpers.mp_blocks, at the oracle's solution (gn_options(4)): (a) np.linalg.inv
of the full information matrix, (b) the device's route restated in NumPy (long_cov_helpers.route_b). Measured values (recorded,
rounded up, in long_cov_helpers.E_REF):

               route a    route b                                  route a    route b
    L65        4.96e-14   4.21e-13  (n = 66)        C129       5.41e-12   7.74e-12  (n = 249)
    L65_angular 2.17e-14  1.47e-12  (n = 66)        W300       9.90e-12   1.33e-10  (n = 243)
    L65_huber  2.57e-14   4.46e-13  (n = 66)        F70        7.38e-11   9.46e-10  (n = 1719)
    MIX        6.14e-12   3.15e-12  (n = 222)       BIG        2.43e-11   2.71e-10  (n = 2763)
    VIO        1.64e-12   1.64e-12  (n = 309)       BANDL      1.88e-11   7.01e-10  (n = 2763)
    C128       5.12e-12   4.46e-11  (n = 249)       KMIX       2.47e-12   1.68e-12  (n = 408, under its prior)

The 50-digit blocks of F70, BIG and BANDL are read from tests/golden/long_cov_ref.npz (scripts/gen_long_cov_golden.py; 45 s, 13 s and
8 s of mpmath); BANDL's are also computed fresh here and must equal the fixture's. The test asserts E_REF / 4 < e <= E_REF: the
recorded bound of the GPU test can neither be exceeded by the reference itself nor have been padded."""
import inspect
import os
import re

import numpy as np
import pytest

import cov_cross_helpers as xh
import cov_helpers as ch
import long_cov_helpers as lc
import long_track_helpers as lh
from sadvio_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_infos = {}


def _info(name, oracle_lib):
    if name not in _infos:
        _infos[name] = lc.oracle_information(name, oracle_lib)
    return _infos[name]


# ---- 1. the yardstick ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in lc.CASES])
def test_float64_routes_against_50_digits(oracle_lib, name):
    info = _info(name, oracle_lib)
    w = info.w
    assert len(lh.long_landmarks(w)) >= 1 and not info.singular
    e_a, e_b, residual = lc.yardstick(name, info)
    e = max(e_a, e_b)
    print(f"[long cov] {name}: n {info.n}, lambda_min {np.linalg.eigvalsh(info.H)[0]:.1e}, e_ref route a {e_a:.3e} route b {e_b:.3e} "
          f"(recorded {lc.E_REF[name]:.1e}), 50-digit residual |H X - I| {residual:.1e}")
    assert residual < 1e-40
    assert lc.E_REF[name] / 4 < e <= lc.E_REF[name], (name, e)


def test_fixture_equals_a_fresh_computation(oracle_lib):
    info = _info("BANDL", oracle_lib)
    fix, _ = lc.mp_reference("BANDL", info)
    fresh, residual = lc.mp_reference("BANDL", info, fresh=True)
    assert residual < 1e-40
    a, b = lc.far_pair(info.w)
    assert np.array_equal(fix["kf"], fresh["kf"]) and np.array_equal(fix["lmk"], fresh["lmk"]) and np.array_equal(fix["cross"](a, b), fresh["cross"](a, b))


@pytest.mark.parametrize("name", lc.CROSS_WINDOWS)
def test_innovation_yardstick(oracle_lib, name):
    """covariance_cross: the newest free key-frame x every landmark. The cross blocks are held to E_REF of the window (asserted here:
    both float64 routes are within it in cov_cross_helpers' norm); the innovation figure has a yardstick of its own, measured as
    tests/test_cov_cross_cpu.py measures its windows', over the same two routes as the blocks (np.linalg.inv | route_b with its cross
    columns -Sigma_pp W^T): MIX 1.25e-12 | 1.15e-12 (n = 222), F70 7.75e-11 | 8.52e-10 (n = 1719)."""
    info = _info(name, oracle_lib)
    w = info.w
    sol = oracle_lib.solve(w, lc.options(name))
    kf, lmk = lc.cross_candidates(w)
    cam, meas = xh.candidate_observations(w, sol, kf, lmk)
    X50 = lc.cross_x50(name, info)
    e_cross = e_innov = 0.0
    for route, X in (("a", np.linalg.inv(info.H)), ("b", lc.route_b(info, full=True))):
        f64 = xh.reference_result(w, info, X, sol, kf, lmk, cam, meas)
        ec, ei = xh.worst_errors(w, info, X50, sol, kf, lmk, cam, meas, f64)
        print(f"[long cov] {name}: {len(kf)} candidates, float64 route {route} against 50 digits: cross norm {ec:.3e} (window's E_REF {lc.E_REF[name]:.1e}), "
              f"innovation {ei:.3e} (recorded {lc.E_REF_INNOV[name]:.1e})")
        e_cross, e_innov = max(e_cross, ec), max(e_innov, ei)
    assert e_cross <= lc.E_REF[name]
    assert lc.E_REF_INNOV[name] / 4 < e_innov <= lc.E_REF_INNOV[name], (name, e_innov)


# ---- 2. the bar sees a defect ----------------------------------------------------------------------------------------------------------
def _drop(w, mask_off):
    keep = np.ones(w.n_obs, dtype=bool)
    keep[mask_off] = False
    return ch._keep_observations(w, keep)


@pytest.mark.parametrize("name", ["MIX", "C129"])
def test_planted_defects_lie_above_the_bar(oracle_lib, name):
    """Four defects a long-track covariance could have, each planted in the reference: the difference from the true blocks must lie
    above 64 x E_REF of the window. C129 has no constant long track: there the fourth defect is planted on a copy whose middle long track
    is constant, against that copy's own blocks."""
    w = lc.window(name)
    sol = oracle_lib.solve(w, lc.options(name))
    info = ch.Information(w, sol, 0.0)
    true = ch.reference_blocks(info)
    pair = [lc.far_pair(w)]
    bar = ch.TOL_FACTOR * lc.E_REF[name]
    longs = [int(l) for l in lh.long_landmarks(w)]
    free_long = [l for l in longs if w.lmk_const is None or not w.lmk_const[l]]
    figures = {}
    # (1) a free long track left out of H altogether: its observations gone, its own block not compared
    l = free_long[-1]
    gone = ch.Information(_drop(w, np.arange(w.lmk_obs_ptr[l], w.lmk_obs_ptr[l + 1])), sol, 0.0)
    assert gone.singular == [l]
    figures["long track left out of H"] = ch.worst_block_difference(ch.reference_blocks(gone), true, gone, pair)
    # (2) the first observation of the second round of 64 dropped
    d2 = ch.Information(_drop(w, [lh.second_round_observation(w, l)]), sol, 0.0)
    figures["observation 64 dropped"] = ch.worst_block_difference(ch.reference_blocks(d2), true, info, pair)
    # (3) one entry's W_e left out of the landmark-block gather of a long track
    k_free = lc.free_kfs(w)
    o = np.arange(w.lmk_obs_ptr[l], w.lmk_obs_ptr[l + 1])
    k_obs = [k for k in k_free if np.any(w.obs_kf[o] == k)]
    figures["one W_e left out of the gather"] = ch.rel_diff(lc.route_b(info, skip_entry=(l, k_obs[0]))["lmk"][l], true["lmk"][l])
    # (4) a constant long track's Jp^T Jp left out of S
    const_long = [q for q in longs if q not in free_long]
    wc, info_c, true_c = w, info, true
    if not const_long:
        const_long = [longs[1]]
        wc = lc.with_const(w, const_long[0])
        sol_c = oracle_lib.solve(wc, lc.options(name))
        info_c = ch.Information(wc, sol_c, 0.0)
        true_c = ch.reference_blocks(info_c)
        sol = sol_c
    q = const_long[0]
    d4 = ch.Information(_drop(wc, np.arange(wc.lmk_obs_ptr[q], wc.lmk_obs_ptr[q + 1])), sol, 0.0)
    figures["constant long track's JpT Jp left out"] = ch.worst_block_difference(ch.reference_blocks(d4), true_c, info_c, pair)
    for what, e in figures.items():
        print(f"[long cov] {name}: {what}: {e:.3e} = {e / bar:.1e} x the bar ({bar:.2e})")
    for what, e in figures.items():
        assert e > bar, (name, what, e, bar)


# ---- 3. flags -------------------------------------------------------------------------------------------------------------------------
def test_flag_matches_the_header_and_the_binding_takes_it():
    hdr = open(os.path.join(ROOT, "include", "sadvio_ba.h")).read()
    m = re.search(r"#define\s+SADVIO_CFG_LONG_TRACK_COVARIANCE\s+(\d+)", hdr)
    assert m and int(m.group(1)) == capi.CFG_LONG_TRACK_COVARIANCE == 4
    for name, val in (("SADVIO_CFG_LONG_TRACKS", capi.CFG_LONG_TRACKS), ("SADVIO_CFG_LONG_TRACK_PRIORS", capi.CFG_LONG_TRACK_PRIORS)):
        assert int(re.search(rf"#define\s+{name}\s+(\d+)", hdr).group(1)) == val
    p = inspect.signature(capi.Backend.__init__).parameters
    assert "long_track_covariance" in p and p["long_track_covariance"].default is False
