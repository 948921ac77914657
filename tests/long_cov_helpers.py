"""Windows with long tracks whose covariances are asked for (sadvio_amd/csrc/cov_long_kernels.h; handles created with
capi.Backend(long_tracks=True, long_track_covariance=True)) and their float64 yardstick: the helper of tests/test_long_cov_cpu.py and
tests/test_gpu_long_cov.py. Every window is built once per process from long_track_helpers / cov_helpers / test_gpu_tile_packing and
never modified (copies carry a changed flag).

The shapes are the smallest at which the long covariance kernels can go wrong:
  L65, L65_angular, L65_huber, MIX, VIO   long_track_helpers.CASES: 65 / 66-70 observations; MIX has a long track at index 0, a constant
          one in the middle and one last; VIO has 15 states per key-frame.
  C128, C129   long_track_helpers.l128(n)'s long tracks 0, 3, 5 first / in the middle / last among 60 five-observation tracks (MIX's
          recipe): two full rounds of 64 observations, and two rounds + 1. (l128 alone is rank deficient for this purpose: its newest
          free key-frames have no observation.)
  W300    300 key-frames, 10 free: one track of 600 observations from all 300 key-frames — more observations and more observing
          key-frames than LONG_THREADS = 256 — between 60 short tracks.
  F70     72 key-frames, 70 free: a 144-observation track seen from every key-frame among 432 four-observation tracks: 70 entries,
          4 900 entry pairs of the landmark block, N_p = 420.
  BIG     long_track_helpers.big(): 80 observations, 40 free key-frames, N_p = 240.
  BANDL   big()'s recipe with the long track seen from the 30 constant key-frames and the 6 oldest free ones: 72 observations on a
          window the band route takes (cov_band_helpers.bandwidth = (5, 36, 6)).
  KMIX    long_prior_helpers' KMIX under its prior, which keeps three long tracks in the reduced system.

E_REF[window] = the largest relative block difference (every key-frame block, one far cross pair, every landmark block) from the
50-digit blocks of cov_helpers.mp_blocks of TWO float64 routes, at the oracle's solution: (a) the inverse of the full information
matrix (cov_helpers.reference_blocks), (b) the device's route restated in NumPy (route_b: eliminate the landmarks, invert S,
Sigma_ll = H_ll^-1 + W Sigma_pp W^T). Route (b) is part of the yardstick because the full inverse alone can come out lucky (3.2e-14 on
L65, a matrix of condition 1e7): a bar of 64 x that could fail a correct kernel. Measured by tests/test_long_cov_cpu.py, which
asserts E_REF / 4 < e <= E_REF; recorded here rounded up. A device block passes at cov_helpers.TOL_FACTOR x E_REF."""
import dataclasses
import os

import numpy as np

import cov_band_helpers as bh
import cov_helpers as ch
import long_track_helpers as lh
import step_helpers as sh
from sadvio_amd import capi, synthetic

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "long_cov_ref.npz")   # scripts/gen_long_cov_golden.py
CROSS_WINDOWS = ("MIX", "F70")             # covariance_cross: the newest free key-frame x every landmark
GOLDEN_WINDOWS = ("F70", "BIG", "BANDL")   # their 50-digit blocks take 45 s, 13 s and 8 s of mpmath


def _well_observed(pool, n=60):
    """The n tracks of the pool with the most observations from the free key-frames, in the pool's order (MIX's recipe)."""
    n_free_obs = np.add.reduceat((pool.kf_const[pool.obs_kf] == 0).astype(int), pool.lmk_obs_ptr[:-1])
    return np.sort(np.argsort(-n_free_obs, kind="stable")[:n])


def c128(n=128):
    import test_gpu_tile_packing as tp
    b = lh.l128(n)
    pool = synthetic.make_window(n_kf=70, n_lmk=600, obs_per_lmk=5, seed=9200, fixed=60)
    assert np.array_equal(pool.kf_T_f_w[pool.kf_const == 1], b.kf_T_f_w[b.kf_const == 1])   # same trajectory
    short = [(pool, int(l), None) for l in _well_observed(pool)]
    w = tp._assemble(pool, [(b, 0, None)] + short[:30] + [(b, 3, None)] + short[30:] + [(b, 5, None)])
    assert lh.long_landmarks(w).tolist() == [0, 31, 62] and lh.counts(w).max() == n
    return w


def w300():
    import test_gpu_tile_packing as tp
    kw = dict(n_kf=300, seed=9700, fixed=290, length=4.0)
    # (a pool of 2 400 tracks: of 600 tracks over 300 key-frames too few see the 10 free ones, and the newest would be left with two landmarks)
    pool = synthetic.make_window(n_lmk=2400, obs_per_lmk=5, **kw)
    b = synthetic.make_window(n_lmk=1, obs_per_lmk=600, **kw)
    assert np.array_equal(pool.kf_T_f_w[pool.kf_const == 1], b.kf_T_f_w[b.kf_const == 1])
    short = [(pool, int(l), None) for l in _well_observed(pool)]
    w = tp._assemble(pool, short[:30] + [(b, 0, None)] + short[30:])
    assert lh.long_landmarks(w).tolist() == [30] and len(np.unique(w.obs_kf[w.lmk_obs_ptr[30]:w.lmk_obs_ptr[31]])) == 300
    return w


def f70():
    import test_gpu_tile_packing as tp
    kw = dict(n_kf=72, seed=9800, fixed=2, length=4.0)
    a = synthetic.make_window(n_lmk=432, obs_per_lmk=4, band=sh.SPREAD, **kw)
    b = synthetic.make_window(n_lmk=1, obs_per_lmk=144, **kw)
    assert np.array_equal(a.kf_T_f_w[a.kf_const == 1], b.kf_T_f_w[b.kf_const == 1])
    w = tp._insert(a, {a.n_lmk // 2: [(b, 0, None)]})
    assert lh.long_landmarks(w).tolist() == [216] and int((w.kf_const == 0).sum()) == 70
    return w


def bandl():
    import test_gpu_tile_packing as tp
    kw = dict(n_kf=70, seed=9500, fixed=30, length=4.0)
    a = synthetic.make_window(n_lmk=70 * 12, obs_per_lmk=4, band=sh.SPREAD, **kw)
    b = synthetic.make_window(n_lmk=1, obs_per_lmk=140, **kw)
    assert np.array_equal(a.kf_T_f_w[a.kf_const == 1], b.kf_T_f_w[b.kf_const == 1])
    w = tp._insert(a, {a.n_lmk // 2: [(b, 0, np.arange(0, 72))]})   # (oldest view first) the 30 constant key-frames and the 6 oldest free ones
    assert lh.counts(w).max() == 72 and bh.bandwidth(w) == (5, 36, 6)
    return w


def kmix_prior():
    import long_prior_helpers as ph
    return ph.case_prior_window(ph.CASE["KMIX"])


@dataclasses.dataclass
class CovCase:
    name: str
    build: object
    huber_a: float = 0.0


CASES = [
    CovCase("L65", lambda: lh.case_window(lh.CASE["L65"])),
    CovCase("L65_angular", lambda: lh.case_window(lh.CASE["L65_angular"])),
    CovCase("L65_huber", lambda: lh.case_window(lh.CASE["L65_huber"]), huber_a=sh.HUBER_A),
    CovCase("MIX", lambda: lh.case_window(lh.CASE["MIX"])),
    CovCase("VIO", lambda: lh.case_window(lh.CASE["VIO"])),
    CovCase("C128", lambda: c128(128)),
    CovCase("C129", lambda: c128(129)),
    CovCase("W300", w300),
    CovCase("F70", f70),
    CovCase("BIG", lambda: lh.case_window(lh.CASE["BIG"])),
    CovCase("BANDL", bandl),
    CovCase("KMIX", kmix_prior),
]
CASE = {c.name: c for c in CASES}
TABLE = [c.name for c in CASES if c.name != "KMIX"]   # the windows every GPU case of the table runs
_windows = {}


def window(name):
    if name not in _windows:
        _windows[name] = CASE[name].build()
    return _windows[name]


def options(name, iters=4):
    o = capi.gn_options(iters)
    if CASE[name].huber_a:
        o.huber_a = CASE[name].huber_a
    return o


def free_kfs(w):
    return [int(k) for k in np.flatnonzero(np.asarray(w.kf_const) == 0)]


def far_pair(w):
    f = free_kfs(w)
    return (f[0], f[-1])


def near_pair(w):
    f = free_kfs(w)
    return (f[0], f[1])


def with_const(w, l):
    """A copy of w whose landmark l is constant."""
    lc = np.zeros(w.n_lmk, dtype=np.uint8) if w.lmk_const is None else np.asarray(w.lmk_const).astype(np.uint8).copy()
    lc[l] = 1
    return dataclasses.replace(w, lmk_const=lc)


def oracle_information(name, oracle_lib, w=None):
    """cov_helpers.Information of the window at the oracle's solution; fails here, on the CPU, when the window is rank deficient."""
    w = window(name) if w is None else w
    sol = oracle_lib.solve(w, options(name), dense_prior=getattr(w, "dense_prior", None))
    info = ch.Information(w, sol, CASE[name].huber_a)
    assert np.linalg.eigvalsh(info.H)[0] > 0, name
    return info


# ---- route (b): the device's route in NumPy ----------------------------------------------------------------------------------------
def route_b(info, skip_entry=None, full=False):
    """Blocks (as Information.blocks_of) by the device's route: S = H_pp - H_pl H_ll^-1 H_lp over the free key-frame states (the landmarks
    eliminated; block by block where no prior couples two of them), Sigma_pp = S^-1, Sigma_ll = H_ll^-1 + W Sigma_pp W^T with
    W = H_ll^-1 H_lp. skip_entry = (landmark, key-frame): the planted defect of the CPU test, that key-frame's W left out of the
    landmark's gather. full: the whole matrix X (landmark blocks on the diagonal only) instead of its blocks."""
    H, n = info.H, info.n
    p = np.concatenate([idx for idx in info.kf_idx if idx is not None])
    is_p = np.zeros(n, bool); is_p[p] = True
    l = np.flatnonzero(~is_p)
    Hll = H[np.ix_(l, l)]
    off = Hll.copy()
    for i in range(0, len(l), 3):
        off[i:i + 3, i:i + 3] = 0.0
    if np.any(off):
        Hi = np.linalg.inv(Hll)
    else:
        Hi = np.zeros_like(Hll)
        for i in range(0, len(l), 3):
            Hi[i:i + 3, i:i + 3] = np.linalg.inv(Hll[i:i + 3, i:i + 3])
    Wl = Hi @ H[np.ix_(l, p)]
    S = H[np.ix_(p, p)] - H[np.ix_(p, l)] @ Wl
    Spp = np.linalg.inv(0.5 * (S + S.T))
    X = np.zeros((n, n))
    X[np.ix_(p, p)] = Spp
    pos_l = {int(c): i for i, c in enumerate(l)}
    pos_p = {int(c): i for i, c in enumerate(p)}
    for li, idx in enumerate(info.lmk_idx):
        if idx is None:
            continue
        r = [pos_l[int(c)] for c in idx]
        Wr = Wl[r].copy()
        if skip_entry is not None and skip_entry[0] == li:
            Wr[:, [pos_p[int(c)] for c in info.kf_idx[skip_entry[1]][:6]]] = 0.0
        X[np.ix_(idx, idx)] = Hi[np.ix_(r, r)] + Wr @ Spp @ Wr.T
    if full:   # with the cross columns Sigma_pl = -Sigma_pp W^T (what k_cov_cross forms)
        X[np.ix_(p, l)] = -Spp @ Wl.T
        X[np.ix_(l, p)] = X[np.ix_(p, l)].T
        return X
    return info.blocks_of(X)


# ---- the 50-digit blocks ------------------------------------------------------------------------------------------------------------
def mp_reference(name, info, fresh=False):
    """(blocks, residual) of cov_helpers.mp_blocks on info: computed, or for GOLDEN_WINDOWS read from the committed fixture (residual
    as recorded by the generator)."""
    if fresh or name not in GOLDEN_WINDOWS:
        return ch.mp_blocks(info, want_residual=True)
    z = np.load(GOLDEN)
    assert np.array_equal(z[f"{name}/H_diag"], np.diag(info.H)), f"{name}: the fixture was made for another matrix"
    a, b = far_pair(info.w)
    far = z[f"{name}/far"]
    blocks = {"kf": z[f"{name}/kf"], "lmk": z[f"{name}/lmk"], "cross": lambda i, j: far if (i, j) == (a, b) else None}
    return blocks, float(z[f"{name}/residual"])


def yardstick(name, info, fresh=False):
    """(e_a, e_b, residual): route (a) and route (b) against the 50-digit blocks."""
    mp, residual = mp_reference(name, info, fresh)
    pair = [far_pair(info.w)]
    e_a = ch.worst_block_difference(ch.reference_blocks(info), mp, info, pair)
    e_b = ch.worst_block_difference(route_b(info), mp, info, pair)
    return e_a, e_b, residual


# ---- covariance_cross: the newest free key-frame x every landmark ------------------------------------------------------------------
def cross_candidates(w):
    return np.full(w.n_lmk, free_kfs(w)[0], dtype=np.int32), np.arange(w.n_lmk, dtype=np.int32)


def cross_x50(name, info, fresh=False):
    """The 50-digit inverse where cross_candidates' candidates read it (cov_cross_helpers.mp_inverse_for): computed, or for a window of
    GOLDEN_WINDOWS rebuilt from the fixture's rows of the newest free key-frame and its landmark blocks."""
    import cov_cross_helpers as xh
    if fresh or name not in GOLDEN_WINDOWS:
        return xh.mp_inverse_for(info, np.arange(info.w.n_lmk))
    z = np.load(GOLDEN)
    assert np.array_equal(z[f"{name}/H_diag"], np.diag(info.H)), f"{name}: the fixture was made for another matrix"
    X = np.zeros((info.n, info.n))
    ia = info.kf_idx[free_kfs(info.w)[0]][:6]
    X[ia, :] = z[f"{name}/xrows"]; X[:, ia] = z[f"{name}/xrows"].T
    for l, idx in enumerate(info.lmk_idx):
        if idx is not None:
            X[np.ix_(idx, idx)] = z[f"{name}/lmk"][l]
    return X


# cov_cross_helpers.worst_errors' innovation figure of the two float64 routes (np.linalg.inv; route_b) against the 50-digit inverse over
# cross_candidates, at the oracle's solution, the larger of the two; measured by tests/test_long_cov_cpu.py, recorded rounded up (the cross
# blocks are held to E_REF of the window)
E_REF_INNOV = {
    "MIX": 1.4e-12,
    "F70": 9.2e-10,
}

# max(route (a), route (b)) against 50 digits, measured by tests/test_long_cov_cpu.py and recorded rounded up
E_REF = {
    "L65": 4.6e-13,
    "L65_angular": 1.6e-12,
    "L65_huber": 4.8e-13,
    "MIX": 6.6e-12,
    "VIO": 1.8e-12,
    "C128": 4.8e-11,
    "C129": 8.4e-12,
    "W300": 1.5e-10,
    "F70": 1.1e-9,
    "BIG": 3.0e-10,
    "BANDL": 7.6e-10,
    "KMIX": 2.7e-12,
}
