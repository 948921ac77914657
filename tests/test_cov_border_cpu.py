"""CPU side of the covariance's border route: the float64 yardsticks of tests/test_gpu_cov_border.py, the arrowhead recursion restated
in NumPy and in 50 digits, and two planted defects that the bar must see. No GPU.

e_ref per window = the largest relative block difference (cov_helpers.rel_diff over every key-frame block, the pairs the GPU test
asks for — inside the core band, core x border, border x border, one core pair outside the band in both orders — and every landmark
block) between np.linalg.inv of the full information matrix and its 50-digit inverse (cov_helpers.mp_blocks), at the oracle's
solution: cov_band_helpers' rule. Measured values (recorded, rounded up, in cov_border_helpers.E_REF):

    closure12          2.11e-12  (N_p = 66, border {1}, hb' 4)         closure12_hb3      2.11e-12  (border {1, 2}, hb' 3)
    revisit12          3.02e-12  (N_p = 66, border {0, 1, 2}, hb' 3)   closure40          5.43e-12  (N_p = 234, border {3}, hb' 7)
    closure_vio8       9.00e-13  (N_p = 105, border {0}, hb' 2)        closure12_angular  4.63e-12
    closure12_huber    2.33e-12
    at_size_closure    1.70e-08  (N_p = 2064, border {5}, hb' 5, cond S 2.3e11; key-frame blocks 1.0e-8, pairs 1.4e-8, landmarks 1.7e-8;
                                 at the oracle's single-threaded solution: with several threads its sums, the state and this figure
                                 move from run to run, 1.2e-8 in one run)

at_size_closure: the float64 side is the block-sparse Schur reference with the closure factor added
(cov_border_helpers.schur_blocks: np.linalg.inv of S), the 50-digit side the arrowhead recursion in mpmath on the same float64
entries (cov_border_helpers.arrowhead_50_digits over cov_band_helpers.mp_band_inverse), for the blocks the GPU test asks for. That
50-digit code is first held against mp_blocks on small windows. Every yardstick test asserts that the day's figure lies in
(E_REF / 4, E_REF]."""
import functools
import os
import re

import numpy as np
import pytest

import cov_band_helpers as cb
import cov_border_helpers as bh
import cov_helpers as ch
from sadvio_amd import capi

SMALL = list(bh.WINDOWS)


@functools.lru_cache(maxsize=None)
def _case(case):
    from oracle import oracle
    oracle.build()
    build, huber, hb = bh.WINDOWS[case]
    w = build()
    opts = capi.reference_options()
    opts.huber_a = huber
    sol = oracle.solve(w, opts)
    info = ch.Information(w, sol, huber)
    plan = bh.plan_of(w, hb)
    kinds = bh.request_pairs(w, plan, every=len(plan.core_of) <= 16)
    return w, sol, huber, info, ch.reference_blocks(info), plan, kinds


@functools.lru_cache(maxsize=None)
def _mp(case):
    return ch.mp_blocks(_case(case)[3], want_residual=True)


def _worst_reduced(got, f64, w, kinds):
    return max([ch.rel_diff(got["kf"][k], f64["kf"][k]) for k in range(w.n_kf)] +
               [ch.rel_diff(got["pair"][i], f64["cross"](a, b)) for i, (a, b) in enumerate(bh.flat_pairs(kinds))])


@pytest.mark.parametrize("case", SMALL)
def test_float64_inverse_against_50_digits(case):
    w, _, _, info, f64, plan, kinds = _case(case)
    mp, residual = _mp(case)
    e = ch.worst_block_difference(f64, mp, info, bh.flat_pairs(kinds))
    print(f"[cov border] {case}: n {info.n}, N_p {info.d * len(plan.core_of)}, border {plan.border}, hb' {plan.hb_core}, e_ref {e:.3e} "
          f"(recorded {bh.E_REF[case]:.1e}), 50-digit residual {residual:.1e}")
    assert residual < 1e-40 and info.singular == []
    assert bh.E_REF[case] / 4 < e <= bh.E_REF[case], (case, e)


@pytest.mark.parametrize("case", SMALL)
def test_arrowhead_recursion_equals_the_full_inverse(case):
    """arrowhead_inverse on the Schur complement against the float64 inverse of the FULL matrix: every key-frame block and every
    pair of the request within the bar of the window (the recursion is another float64 route to the same numbers, so it is held to
    what a device block is held to). Blocks inside the core band and on the border are symmetric to the bit."""
    w, _, _, info, f64, plan, kinds = _case(case)
    S, _ = cb.schur(info)
    X, parts = bh.arrowhead_inverse(S, plan, info.d, cb.block_column(info.d))
    got = bh.reduced_blocks(w, plan, X, parts, kinds)
    e = _worst_reduced(got, f64, w, kinds)
    print(f"[cov border] {case}: arrowhead recursion against the full inverse {e:.3e}; bound {ch.TOL_FACTOR * bh.E_REF[case]:.3e}")
    assert e <= ch.TOL_FACTOR * bh.E_REF[case]
    # what the route forms and nothing else: the core band, the border's rows and columns
    p, nc, d = parts["p"], parts["nc"], info.d
    formed = ~np.isnan(X[np.ix_(p, p)])
    i, j = np.indices(formed.shape)
    assert np.array_equal(formed, (i >= nc) | (j >= nc) | (np.abs(i // d - j // d) <= plan.hb_core))


@pytest.mark.parametrize("case", ["closure12", "revisit12"])
def test_50_digit_arrowhead_against_mp_blocks(case):
    """arrowhead_50_digits on the float64 Schur complement against mp_blocks of the full matrix: the two 50-digit routes start from
    different float64 entries (S is rounded once more), so they agree within the window's e_ref, not to 1e-14."""
    w, _, _, info, _, plan, kinds = _case(case)
    mp, _ = _mp(case)
    S, cols = cb.schur(info)
    d = info.d
    pairs = bh.flat_pairs(kinds)
    blocks = [(k, k) for k in range(w.n_kf) if cols[k] >= 0] + pairs
    want = [(int(cols[a]) + r, int(cols[b]) + s) for a, b in blocks for r in range(d) for s in range(d)]
    got = bh.arrowhead_50_digits(bh.dense_entries(S), S.shape[0], plan, d, want)
    e = 0.0
    for a, b in blocks:
        blk = np.array([[got[(int(cols[a]) + r, int(cols[b]) + s)] for s in range(d)] for r in range(d)])
        e = max(e, ch.rel_diff(blk, mp["kf"][a] if a == b else mp["cross"](a, b)))
    print(f"[cov border] {case}: 50-digit arrowhead against mp_blocks {e:.3e}; e_ref {bh.E_REF[case]:.1e}")
    assert e <= bh.E_REF[case]


@pytest.mark.parametrize("case", ["closure12", "revisit12", "closure40", "closure12_angular", "closure12_huber"])
@pytest.mark.parametrize("defect", ["drop_zw_block", "skip_l_row"])
def test_planted_defects_miss_the_bar(case, defect):
    """One in-band block of Sigma_BB (the diagonal block of the core's middle key-frame) without its Z W^T correction, or the first
    border column solved with one row of L ignored (the last but one core row, where the forward substitution has met every
    non-zero of the column), misses the bar on every VO window: the bar sees such a defect. A T that the defect leaves indefinite
    counts as seen."""
    w, _, _, info, f64, plan, kinds = _case(case)
    S, _ = cb.schur(info)
    d = info.d
    kw = dict(drop_zw_block=(plan.n_core // 2, plan.n_core // 2)) if defect == "drop_zw_block" else dict(skip_l_row=plan.n_core * d - 2)
    try:
        X, parts = bh.arrowhead_inverse(S, plan, d, cb.block_column(d), **kw)
        e = _worst_reduced(bh.reduced_blocks(w, plan, X, parts, kinds), f64, w, kinds)
    except np.linalg.LinAlgError:
        e = np.inf
    print(f"[cov border] {case}: {defect} {e:.3e}; bound {ch.TOL_FACTOR * bh.E_REF[case]:.3e}")
    assert e > ch.TOL_FACTOR * bh.E_REF[case]


def at_size_request(w, plan):
    """The blocks tests/test_gpu_cov_border.py asks of the at-size closure window."""
    a, b = bh.AT_SIZE_CLOSURE_KF
    kf, _, lmk = cb.at_size_request(w, plan.hb_core)
    return kf + [a, b], [(172, 173), (173, 172), (4, 6), (4, 5), (5, 6), (a, b), (b, a), (3, 339), (339, 3)], lmk


def test_at_size_closure_float64_schur_reference_against_50_digits():
    """The 345-key-frame window with its closure factor: S stays positive definite at window_at_size's seed (smallest eigenvalue
    printed and asserted), the border is key-frame 5, and the blocks the GPU test asks for (key-frames, pairs, 20 landmarks) agree
    between the float64 Schur reference (np.linalg.inv of S) and the 50-digit side within the recorded e_ref. The 50-digit side
    starts from the same float64 entries of H: S is formed in 50 digits, then the arrowhead recursion, then the landmark blocks."""
    import mpmath
    from oracle import oracle
    oracle.build()
    w = bh.window_at_size_closure()
    sol = oracle.solve(w, capi.reference_options(), n_threads=1)      # (one thread: the same sums, so the same state and the same figure, every run)
    sb = bh.schur_blocks(w, sol)
    plan = bh.plan_of(w)
    assert plan.answer == "OK" and plan.border == [bh.AT_SIZE_CLOSURE_KF[0]] and sb.n == 2064
    ev = np.linalg.eigvalsh(sb.S())
    kf, pairs, lmk = at_size_request(w, plan)
    f64 = sb.blocks(kf, pairs, lmk)
    c = sb.cols
    blocks = [(k, k) for k in kf] + pairs
    want = {(int(c[a]) + r, int(c[b]) + s) for a, b in blocks for r in range(6) for s in range(6)}
    for l in lmk:
        want |= {(int(ra), int(rb)) for ra in sb.rows[l] for rb in sb.rows[l]}
    S50, recs = bh.schur_entries_50_digits(sb, lmk)
    got = bh.arrowhead_50_digits(S50, sb.n, plan, 6, sorted(want), as_float=False)
    e = {"kf": 0.0, "pair": 0.0, "lmk": 0.0}
    for q, (a, b) in enumerate(blocks):
        blk = np.array([[float(got[(int(c[a]) + r, int(c[b]) + s)]) for s in range(6)] for r in range(6)])
        key = "kf" if q < len(kf) else "pair"
        e[key] = max(e[key], ch.rel_diff(f64[key][q if q < len(kf) else q - len(kf)], blk))
    for q, l in enumerate(lmk):
        Di, BD = recs[l]
        rows = [int(r) for r in sb.rows[l]]
        sub = mpmath.matrix([[got[(ra, rb)] for rb in rows] for ra in rows])
        blk = Di + BD.T * sub * BD
        e["lmk"] = max(e["lmk"], ch.rel_diff(f64["lmk"][q], np.array([[float(blk[r, s]) for s in range(3)] for r in range(3)])))
    worst = max(e.values())
    print(f"[cov border] at_size_closure: N_p {sb.n}, border {plan.border}, hb' {plan.hb_core}, smallest eigenvalue of S {ev[0]:.3e}, cond S {ev[-1] / ev[0]:.2e}, "
          f"e_ref kf {e['kf']:.3e} pair {e['pair']:.3e} lmk {e['lmk']:.3e} (recorded {bh.E_REF['at_size_closure']:.1e})")
    assert ev[0] > 0
    assert bh.E_REF["at_size_closure"] / 4 < worst <= bh.E_REF["at_size_closure"], worst


def test_route_constant_matches_the_c_header():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sadvio_ba.h")).read()
    m = re.search(r"#define\s+SADVIO_COV_ROUTE_BORDER\s+(\d+)", hdr)
    assert m and int(m.group(1)) == capi.COV_ROUTE_BORDER == 4
