"""Windows and yardsticks of the sadvio_ba_covariance_batch tests (test infrastructure; the reference side is cov_helpers').

The windows tests/test_gpu_cov.py already measures keep their cov_helpers.E_REF. The five below are new: two plain VO windows and
an angular one for the batches the throughput kernels solve, and the pair that straddles the cap of the in-LDS inverse
(N_p <= 176): 29 free key-frames (N_p = 174, the largest window on the LDS route) and 30 (N_p = 180, the smallest on the dense
route). E_REF here is measured as cov_helpers.E_REF is — the float64 inverse of the full information matrix against the 50-digit
one at the oracle's solution, tests/test_cov_batch_cpu.py — and recorded rounded up; a device block passes at TOL_FACTOR x E_REF."""
import cov_helpers as ch
from sadvio_amd import capi, synthetic

WINDOWS = {   # case -> (builder, cross pair of the CPU measurement)
    "w7": (lambda: synthetic.make_window(n_kf=6, n_lmk=400, seed=7), (0, 4)),
    "w42": (lambda: synthetic.make_window(n_kf=5, n_lmk=300, seed=42), (0, 3)),
    "w7_angular": (lambda: synthetic.make_window(n_kf=6, n_lmk=400, seed=7, factor=capi.FACTOR_ANGULAR), (0, 4)),
    "np174": (lambda: synthetic.make_window(n_kf=30, n_lmk=300, obs_per_lmk=8, seed=207, length=6.0), (0, 28)),
    "np180": (lambda: synthetic.make_window(n_kf=31, n_lmk=300, obs_per_lmk=8, seed=208, length=6.0), (0, 29)),
}
N_P = {"w7": 30, "w42": 24, "w7_angular": 30, "np174": 174, "np180": 180}

# measured by test_cov_batch_cpu.py::test_float64_inverse_against_50_digits (the figures are in its docstring)
E_REF = dict(ch.E_REF)
E_REF.update({
    "w7": 9.6e-13,
    "w42": 3.1e-13,
    "w7_angular": 1.6e-12,
    "np174": 3.3e-12,
    "np180": 7.1e-12,
})


def window(case):
    return WINDOWS[case][0]()


def n_p(w):
    """Columns of the reduced system of a window without prior-kept landmarks."""
    return (15 if w.has_imu else 6) * int((w.kf_const == 0).sum())


def unit_bytes(w):
    """Work arrays of one window in a group of the batch call (cov_batch_driver.h: per landmark 21 doubles + 2 ints, per observation
    39 doubles + 1 int, S and Sigma_pp)."""
    nn = max(n_p(w), 1) ** 2
    return 8 * (21 * w.n_lmk + 39 * w.n_obs + 2 * nn) + 4 * (2 * w.n_lmk + w.n_obs + 1)


_REF_CACHE = {}


def check_item(case, w, d, c, huber=0.0, pairs=(), kf=None, lmk="all", w_ref=None, tag=""):
    """The blocks of one batch item c (key-frames `kf`, cross `pairs`, landmarks `lmk`: a list or "all") against the float64 inverse of
    the full information matrix at the deltas d; bar TOL_FACTOR x E_REF[case]. Prints the worst figure, then asserts. The reference
    of a (case, deltas) is computed once and shared. Returns the worst relative block difference."""
    import numpy as np
    key = (case, huber, d["pose"].tobytes(), d["lmk"].tobytes())
    if key not in _REF_CACHE:
        info = ch.Information(w_ref if w_ref is not None else w, d, huber)
        _REF_CACHE[key] = (info, ch.reference_blocks(info))
    info, ref = _REF_CACHE[key]
    tol = ch.TOL_FACTOR * E_REF[case]
    worst = {"kf": 0.0, "pair": 0.0, "lmk": 0.0}
    for i, k in enumerate(kf or []):
        worst["kf"] = max(worst["kf"], ch.rel_diff(c["kf"][i], ref["kf"][k]))
    for i, (a, b) in enumerate(pairs):
        worst["pair"] = max(worst["pair"], ch.rel_diff(c["pair"][i], ref["cross"](a, b)))
    lm = list(range(w.n_lmk)) if isinstance(lmk, str) else list(lmk or [])
    n_sing = 0
    for i, l in enumerate(lm):
        if l in info.singular:
            n_sing += 1
            assert np.isnan(c["lmk"][i]).all(), l
        else:
            assert np.isfinite(c["lmk"][i]).all(), l
            worst["lmk"] = max(worst["lmk"], ch.rel_diff(c["lmk"][i], ref["lmk"][l]))
    print(f"[cov batch] {case}{tag}: route {c.get('route')}, worst relative block difference kf {worst['kf']:.3e} pair {worst['pair']:.3e} "
          f"lmk {worst['lmk']:.3e}; bound {tol:.3e} (64 x e_ref {E_REF[case]:.1e})")
    assert c["n_lmk_singular"] == n_sing
    assert max(worst.values()) <= tol, (case, worst, tol)
    return max(worst.values())


def same_bytes(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in ("kf", "pair", "lmk")) and a["n_lmk_singular"] == b["n_lmk_singular"]


def worst_difference(a, b):
    """Largest relative block difference between two results of the same request (NaN blocks must coincide)."""
    import numpy as np
    worst = 0.0
    for k in ("kf", "pair", "lmk"):
        for x, y in zip(a[k], b[k]):
            if np.isnan(y).any():
                assert np.isnan(x).all()
                continue
            worst = max(worst, ch.rel_diff(x, y))
    return worst
