"""CPU side of the covariance's band route: the float64 yardsticks of tests/test_gpu_cov_band.py, the bandwidth rule, the selected
inversion restated in NumPy and two planted defects that the bar must see. No GPU.

e_ref per window = the largest relative block difference (cov_helpers.rel_diff over every key-frame block, every in-band pair, the
pair of the two outermost free key-frames in both orders, every landmark block) between np.linalg.inv of the full information
matrix and its 50-digit inverse (cov_helpers.mp_blocks), at the oracle's solution. Measured values (recorded, rounded up, in
cov_band_helpers.E_REF):

    vo12          5.22e-12  (N_p = 66,  bw = 30)      relpose  2.11e-12  (N_p = 66,  bw = 48)
    vo12_angular  4.52e-12  (N_p = 66,  bw = 30)      huber    1.47e-12  (N_p = 66,  bw = 30)
    vo40          9.19e-12  (N_p = 234, bw = 54)      vio8     8.94e-13  (N_p = 105, bw = 45)
    at_size       6.96e-08  (N_p = 2064, bw = 36, cond S 1.5e12: a chain of 344 free key-frames anchored at one end)

at_size: the full matrix has 11 379 columns; the float64 side is the block-sparse Schur reference (cov_band_helpers.SchurBlocks:
np.linalg.inv of S, Sigma_ll through W_l), the 50-digit side the band Cholesky factor and the Takahashi recursion in mpmath on the
same float64 entries, for the blocks the GPU test asks for. That 50-digit band code is first held against mp_blocks on small windows.
Every test asserts that the day's figure lies in (E_REF / 4, E_REF]."""
import functools

import numpy as np
import pytest

import cov_band_helpers as cb
import cov_helpers as ch
from sadvio_amd import capi

SMALL = list(cb.WINDOWS)


def yardstick_pairs(w, hb):
    f = cb.free_index(w)
    free = [k for k in range(w.n_kf) if f[k] >= 0]
    return cb.in_band_pairs(w, hb) + [(free[0], free[-1]), (free[-1], free[0])]


@functools.lru_cache(maxsize=None)
def _case(case):
    from oracle import oracle
    oracle.build()
    build, huber = cb.WINDOWS[case]
    w = build()
    opts = capi.reference_options()
    opts.huber_a = huber
    sol = oracle.solve(w, opts)
    info = ch.Information(w, sol, huber)
    return w, sol, huber, info, ch.reference_blocks(info)


@functools.lru_cache(maxsize=None)
def _mp(case):
    return ch.mp_blocks(_case(case)[3], want_residual=True)


@pytest.mark.parametrize("case", SMALL)
def test_float64_inverse_against_50_digits(case):
    w, _, _, info, f64 = _case(case)
    hb, bw, dpf = cb.bandwidth(w)
    mp, residual = _mp(case)
    e = ch.worst_block_difference(f64, mp, info, yardstick_pairs(w, hb))
    print(f"[cov band] {case}: n {info.n}, N_p {dpf * int((cb.free_index(w) >= 0).sum())}, hb {hb}, bw {bw}, e_ref {e:.3e} "
          f"(recorded {cb.E_REF[case]:.1e}), 50-digit residual {residual:.1e}")
    assert residual < 1e-40 and info.singular == []
    assert cb.E_REF[case] / 4 < e <= cb.E_REF[case], (case, e)


@pytest.mark.parametrize("case", ["vo12", "huber"])
def test_50_digit_band_code_against_mp_blocks(case):
    """SchurBlocks.blocks_50_digits (landmark blocks, band Cholesky, recursion, band substitution for the pair outside the band) on
    a window small enough for mp_blocks: with one chunk its float64 entries are Information's, and the two 50-digit routes agree to
    the rounding of their float64 output."""
    w, sol, huber, info, _ = _case(case)
    hb, bw, _ = cb.bandwidth(w)
    mp, _ = _mp(case)
    sb = cb.SchurBlocks(w, sol, huber, chunk=w.n_lmk)
    assert np.array_equal(sb.S(), sb.S().T)
    kf, pairs, lmk = list(range(w.n_kf)), [(0, 2), (2, 0), (0, 10), (10, 0), (3, 9)], list(range(w.n_lmk))
    got = sb.blocks_50_digits(bw, kf, pairs, lmk)
    ref = {"kf": mp["kf"], "pair": [mp["cross"](a, b) for a, b in pairs], "lmk": mp["lmk"]}
    e = cb.worst(got, ref)
    print(f"[cov band] {case}: 50-digit band code against mp_blocks {e:.3e}")
    assert e < 1e-14
    # ... and in several chunks the float64 entries of H_pp are summed in another order: within the window's e_ref
    e2 = cb.worst(cb.SchurBlocks(w, sol, huber, chunk=64).blocks_50_digits(bw, kf, pairs, lmk), ref)
    print(f"[cov band] {case}: in chunks of 64 landmarks {e2:.3e}")
    assert e2 <= cb.E_REF[case]


@functools.lru_cache(maxsize=1)
def _at_size():
    from oracle import oracle
    oracle.build()
    w = cb.window_at_size()
    sol = oracle.solve(w, capi.reference_options(), n_threads=8)
    return w, cb.SchurBlocks(w, sol)


def test_at_size_float64_schur_reference_against_50_digits():
    w, sb = _at_size()
    hb, bw, dpf = cb.bandwidth(w)
    assert (sb.n, dpf) == (2064, 6) and bw < sb.n and sb.n + 1 > 2047
    kf, pairs, lmk = cb.at_size_request(w, hb)
    f = cb.free_index(w)
    assert abs(f[pairs[0][0]] - f[pairs[0][1]]) <= hb < abs(f[pairs[1][0]] - f[pairs[1][1]]) and len(lmk) == 20
    f64 = sb.blocks(kf, pairs, lmk)
    mp = sb.blocks_50_digits(bw, kf, pairs, lmk)
    e = cb.worst(f64, mp)
    ev = np.linalg.eigvalsh(sb.S())
    print(f"[cov band] at_size: N_p {sb.n}, hb {hb}, bw {bw}, cond S {ev[-1] / ev[0]:.2e}, e_ref {e:.3e} (recorded {cb.E_REF['at_size']:.1e})")
    assert ev[0] > 0
    assert cb.E_REF["at_size"] / 4 < e <= cb.E_REF["at_size"], e


@pytest.mark.parametrize("case", SMALL + ["at_size"])
def test_bandwidth_rule(case):
    """The NumPy S of every window has no non-zero outside the band the rule predicts, and the band is not wider than needed: the
    last block diagonal inside it is not all zero."""
    if case == "at_size":
        w, sb = _at_size()
        S = sb.S()
    else:
        w, _, _, info, _ = _case(case)
        S, _ = cb.schur(info)
    hb, bw, dpf = cb.bandwidth(w)
    n = S.shape[0]
    assert bw == (hb + 1) * dpf < n
    i, j = np.indices(S.shape)
    assert not np.any(S[np.abs(i - j) >= bw])
    assert np.any(S[(np.abs(i - j) >= bw - dpf) & (np.abs(i - j) < bw)])


@pytest.mark.parametrize("case", SMALL)
def test_recursion_equals_the_full_inverse(case):
    """band_selected_inverse on the Schur complement against the float64 inverse of the FULL matrix: every key-frame block and
    every in-band pair within the bar of the window (the recursion is another float64 route to the same numbers, so it is held to
    what a device block is held to)."""
    w, _, _, info, f64 = _case(case)
    hb, bw, dpf = cb.bandwidth(w)
    S, cols = cb.schur(info)
    pairs = cb.in_band_pairs(w, hb)
    got = cb.blocks_of_reduced(info, cb.band_selected_inverse(S, bw, cb.block_column(dpf)), cols, pairs)
    assert np.isfinite(got["kf"]).all() and np.isfinite(got["pair"]).all()      # everything asked for lies inside the band
    e = max([ch.rel_diff(got["kf"][k], f64["kf"][k]) for k in range(w.n_kf)] + [ch.rel_diff(got["pair"][i], f64["cross"](a, b)) for i, (a, b) in enumerate(pairs)])
    print(f"[cov band] {case}: recursion against the full inverse {e:.3e}; bound {ch.TOL_FACTOR * cb.E_REF[case]:.3e}")
    assert e <= ch.TOL_FACTOR * cb.E_REF[case]
    for k in range(w.n_kf):
        assert np.array_equal(got["kf"][k], got["kf"][k].T)


@pytest.mark.parametrize("case", ["vo12", "vo12_angular", "vo40", "relpose", "huber"])
@pytest.mark.parametrize("defect", ["drop_last_block_row", "bw_minus_nb"])
def test_planted_defects_miss_the_bar(case, defect):
    """A recursion whose J is one block row short, or that runs with bw - nb, misses the bar on every VO window: the bar sees such
    a defect. (On the VIO window the last nb rows of the band are bias rows of the furthest key-frame, which only the IMU pair of
    neighbouring frames couples: bw - nb loses nothing there, so that window is left out.)"""
    w, _, _, info, f64 = _case(case)
    hb, bw, dpf = cb.bandwidth(w)
    nb = cb.block_column(dpf)
    S, cols = cb.schur(info)
    X = cb.band_selected_inverse(S, bw, nb, True) if defect == "drop_last_block_row" else cb.band_selected_inverse(S, bw - nb, nb)
    got = cb.blocks_of_reduced(info, X, cols)
    e = max(ch.rel_diff(got["kf"][k], f64["kf"][k]) for k in range(w.n_kf))
    print(f"[cov band] {case}: {defect} {e:.3e}; bound {ch.TOL_FACTOR * cb.E_REF[case]:.3e}")
    assert e > ch.TOL_FACTOR * cb.E_REF[case]


def test_route_constant_matches_the_c_header():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sadvio_ba.h")).read()
    m = re.search(r"#define\s+SADVIO_COV_ROUTE_BAND\s+(\d+)", hdr)
    assert m and int(m.group(1)) == capi.COV_ROUTE_BAND == 3
