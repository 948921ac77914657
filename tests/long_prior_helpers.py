"""Windows whose long tracks (landmarks of more than 64 observations) are marginalised, sparsified and kept in the reduced system by
priors: the helper of tests/test_long_prior_cpu.py, tests/test_long_prior_plan_cpu.py and tests/test_gpu_long_priors.py. Handles that
serve them are created with capi.Backend(long_tracks=True, long_track_priors=True) (SADVIO_CFG_LONG_TRACKS | SADVIO_CFG_LONG_TRACK_PRIORS).

Every window is built once per process and never modified (copies carry the priors). The shapes are the smallest at which the new
branches can go wrong:

  KL65   long_track_helpers.l65(): 34 key-frames, 29 constant, 12 landmarks of 65 observations. The oldest key-frame (index n_kf - 1)
         sees 8 of them in stereo: pre_marginalize keeps 5 and marginalises none (every kept landmark is a long track).
  KMIX   34 key-frames, 28 constant, seed 9600: 120 landmarks of 5 observations with 66-observation landmarks in front of landmark 0,
         two adjacent ones in the middle and one behind the last: tiles and long tracks under one prior. pre_marginalize keeps 6
         landmarks, 3 of them long.
  KVIO   long_track_helpers.vio_long()'s shape (36 key-frames, 6 free, 15 states each) whose 66-observation landmark is seen from the
         oldest key-frame in stereo: kept beside the kept frame's 15 columns (kf_keep = n_kf - 2, marg_has_imu); 4 landmarks kept.
  KBIG   long_track_helpers.big() (70 key-frames, 40 free) under a full-rank random prior (test_gpu_prior.random_prior's scaling) that
         keeps its 80-observation landmark and two 4-observation ones: N_p = 249 > 174, the reduced system with the prior's columns is
         solved out of LDS.
  K258   134 key-frames, 128 constant, 4 landmarks of 258 observations, a random prior keeps two of them: more observations than
         LONG_THREADS = 256, so a kept track runs the long kernels' second round (they linearise twice: the `!single` path). This
         stands in for the issue's KL129, whose 129 observations stay within one round.

E_REF[case] = step_error(oracle's float64 first step, 50-digit step) under the case's prior, measured by tests/test_long_prior_cpu.py
and recorded here 1.5 x the measured value rounded up, as tests/long_track_helpers.py does; a device step passes at
TOL_FACTOR x max(E_REF, FLOOR) of step_helpers."""
import dataclasses
import os

import numpy as np

import long_track_helpers as lh
import step_helpers as sh
from sadvio_amd import capi, synthetic

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "long_prior_first_step_ref.npz")   # make_golden_long_prior_first_step.py
PRIOR_KEYS = ("J", "r0", "kf_keep", "kf_col", "lmk_index", "lmk_col")


def kl65(factor=lh.PIXEL, **kw):
    return lh.l65(factor, **kw)


def kmix():
    import test_gpu_tile_packing as tp
    kw = dict(n_kf=34, seed=9600, fixed=28)
    a = synthetic.make_window(n_lmk=120, obs_per_lmk=5, **kw)
    b = synthetic.make_window(n_lmk=12, obs_per_lmk=66, **kw)
    assert np.array_equal(a.kf_T_f_w[a.kf_const == 1], b.kf_T_f_w[b.kf_const == 1])   # same trajectory
    kf0 = a.n_kf - 1
    stereo = [l for l in range(b.n_lmk) if (b.obs_kf[b.lmk_obs_ptr[l]:b.lmk_obs_ptr[l + 1]] == kf0).sum() == 2]
    other = [l for l in range(b.n_lmk) if l not in stereo]
    assert len(stereo) >= 3 and other
    # in front of landmark 0 and the second of the middle pair: seen from the oldest key-frame in stereo (kept); the first of the pair: not
    # seen from it (a free long track beside the kept ones); the last: kept
    w = tp._insert(a, {0: [(b, stereo[0], None)], 60: [(b, other[0], None), (b, stereo[1], None)]})
    picks = [(w, l, None) for l in range(w.n_lmk)] + [(b, stereo[2], None)]
    w = tp._assemble(w, picks)
    assert lh.long_landmarks(w).tolist() == [0, 61, 62, 123] and w.n_lmk == 124
    return w


def kvio():
    """long_track_helpers.vio_long()'s shape (36 key-frames, 6 free, 15 states each, 4-observation landmarks) whose one 66-observation
    landmark is seen from the oldest key-frame in stereo: the marginalisation keeps it beside the kept frame's 15 columns."""
    import test_gpu_tile_packing as tp
    from vio_helpers import make_vio_window
    a = make_vio_window(n_kf=36, n_lmk=72, obs_per_lmk=4, seed=9400, fixed=30)
    b = synthetic.make_window(n_kf=36, n_lmk=12, obs_per_lmk=66, seed=9400, fixed=30)
    assert np.array_equal(a.kf_T_f_w[a.kf_const == 1], b.kf_T_f_w[b.kf_const == 1])
    kf0 = a.n_kf - 1
    stereo = [l for l in range(b.n_lmk) if (b.obs_kf[b.lmk_obs_ptr[l]:b.lmk_obs_ptr[l + 1]] == kf0).sum() == 2]
    b_free = np.add.reduceat((b.kf_const[b.obs_kf] == 0).astype(int), b.lmk_obs_ptr[:-1])
    pick = max(stereo, key=lambda l: b_free[l])
    w = lh._carry(tp._insert(a, {40: [(b, int(pick), None)]}), a)
    assert lh.long_landmarks(w).tolist() == [40] and b_free[pick] >= 2
    return w


def vio_marg_args(w):
    """The marginalisation of the oldest key-frame of a VIO window: its IMU factor to the next one, which is kept, on top of a previous
    prior on the marginalised frame's 15 states (the construction of test_gpu_sparsify.py's pipeline test; a sliding back end always
    has one). Without it nothing but the IMU factor holds that frame's velocity and biases, the marginal on the kept frame's 15
    columns is singular (rank 19 of 27 on KVIO, cond of its covariance block 3e17) and sparsifyVIO's IMU prior factor, which inverts
    that block, is not a defined quantity: tests/test_long_prior_cpu.py measures both."""
    kf0, kf1 = w.n_kf - 1, w.n_kf - 2
    keep, marg = synthetic.pre_marginalize(w, kf0)
    imu = [f for f in w.imu_factors if f["kf_i"] == kf0 and f["kf_j"] == kf1][0]
    rng = np.random.default_rng(9400)
    last = {"J": 20.0 * (np.eye(15) + 0.1 * rng.standard_normal((15, 15))), "r0": 0.1 * rng.standard_normal(15), "kf_keep": kf0, "kf_col": 0,
            "lmk_index": np.zeros(0, dtype=np.int32), "lmk_col": np.zeros(0, dtype=np.int32)}
    return dict(kf_marg=kf0, lmk_marg=marg, lmk_keep=keep, kf_keep=kf1, marg_has_imu=True, imu=imu, priors=list(w.pose_priors), last=last)


LONG_FACTOR_RAISE = 4.0


def raise_long_factor(factors, long_, k=LONG_FACTOR_RAISE):
    """The sparsified factors with the square-root information of the pose-to-landmark factor on landmark long_ multiplied by k. On
    KVIO the kept frame is constant and sparsifyVIO's factor anchors the long track where it was linearised: dropped, it moves the
    oracle's poses by 7.5e-6, less than 10 x the pose bar of the pipeline test (1e-6). With its information raised 16-fold (k = 4) the
    dropped factor moves them by 1.2e-4 (tests/test_long_prior_cpu.py), so the pose bar sees it."""
    return [dict(f, sqrt_inf=np.asarray(f["sqrt_inf"]) * k) if f["type"] == capi.SPARSE_POSE_TO_LMK and f["lmk0"] == long_ else f for f in factors]


def kept_frame_covariance_cond(prior):
    """(rank, n, condition number of the kept frame's 15 x 15 block of Sigma_k = pinv(J^T J), eigenvalues cut at the reference's 1e-12):
    the block that sparsifyVIO's IMU prior factor inverts."""
    H = prior["J"].T @ prior["J"]
    ev = np.linalg.eigvalsh(H)
    Sk = np.linalg.pinv(H, rcond=1e-12 / ev[-1], hermitian=True)
    c = int(prior["kf_col"])
    return int((ev > 1e-12).sum()), H.shape[0], float(np.linalg.cond(Sk[c:c + 15, c:c + 15]))


def marg_args(w):
    """The marginalisation of the oldest key-frame of a VO window under the reference's selection rule."""
    kf0 = w.n_kf - 1
    keep, marg = synthetic.pre_marginalize(w, kf0)
    return dict(kf_marg=kf0, lmk_marg=marg, lmk_keep=keep, priors=list(getattr(w, "pose_priors", None) or []))


def next_window(w, prior):
    """The window after the marginalisation of its oldest key-frame: the same arrays, that key-frame constant, under `prior`."""
    return dataclasses.replace(w, dense_prior={k: prior[k] for k in PRIOR_KEYS if k in prior}, _keep=[])


def sparse_window(w, factors):
    """... under the sparsified prior instead."""
    return dataclasses.replace(w, sparse_priors=factors, _keep=[])


def with_oracle_prior(w, oracle_lib, args=None):
    o = oracle_lib.marginalize(w, **(args or marg_args)(w))
    assert o is not None
    return next_window(w, o)


def p2l_factor(w, l, kf, pull=0.05, inf=8.0):
    """A pose-to-landmark factor of the sparse prior between key-frame kf and landmark l whose measurement lies `pull` beside the
    landmark's position in the frame, so that the factor moves the solution."""
    from sparse_helpers import spd_sqrt
    T = np.asarray(w.kf_T_f_w[kf])
    return {"type": capi.SPARSE_POSE_TO_LMK, "kf": kf, "lmk0": l, "delta": T[:9].reshape(3, 3) @ w.lmk_p[l] + T[9:] + pull,
            "sqrt_inf": spd_sqrt(np.random.default_rng(3), 3, inf)}


def p2l_windows():
    """(name, window, its pose-to-landmark factor on a free long track): KMIX (VO; landmark 61, which no prior keeps, from the newest
    key-frame) and long_track_helpers.vio_long() (15 states per key-frame; its 66-observation landmark from the oldest free key-frame)."""
    km, vio = case_window(CASE["KMIX"]), lh.case_window(lh.CASE["VIO"])
    kf_vio = int(np.flatnonzero(np.asarray(vio.kf_const) == 0).max())
    return [("KMIX", km, p2l_factor(km, 61, 0)), ("VIO", vio, p2l_factor(vio, int(lh.long_landmarks(vio)[0]), kf_vio))]


def random_prior(w, lmk_index, seed, scale=3.0):
    """A full-rank random dense prior on the landmarks lmk_index (no kept frame): J = scale * N(0, 1) / sqrt(n), as
    test_gpu_prior.random_prior scales it."""
    rng = np.random.default_rng(seed)
    n = 3 * len(lmk_index)
    return {"J": scale * rng.standard_normal((n, n)) / np.sqrt(n), "r0": 0.5 * rng.standard_normal(n), "kf_keep": -1, "kf_col": 0,
            "lmk_index": np.array(lmk_index, dtype=np.int32), "lmk_col": (3 * np.arange(len(lmk_index))).astype(np.int32)}


def k258():
    return synthetic.make_window(n_kf=134, n_lmk=4, obs_per_lmk=258, seed=9700, fixed=128)


def kbig_prior(w):
    return random_prior(w, [5, int(lh.long_landmarks(w)[0]), w.n_lmk - 7], 9800)


@dataclasses.dataclass
class PriorCase:
    name: str
    build: object                 # () -> window without its prior
    n_keep: int                   # landmarks the prior keeps
    n_keep_long: int              # ... of them long tracks
    opts: dict = dataclasses.field(default_factory=dict)
    window: str = ""
    prior: object = None          # (window) -> its dense prior; None: the oracle's marginalisation of the oldest key-frame
    marg: object = None           # (window) -> the arguments of that marginalisation; None: marg_args (VO)

    def __post_init__(self):
        self.window = self.window or self.name


CASES = [
    PriorCase("KL65", kl65, 5, 5),
    PriorCase("KMIX", kmix, 6, 3),
    PriorCase("KL65_angular", lambda: kl65(lh.ANGULAR), 5, 5),
    PriorCase("KL65_huber", lambda: kl65(**sh.SMALL_PERTURB), 5, 5, opts={"huber_a": sh.HUBER_A}),
    PriorCase("KVIO", kvio, 4, 1, marg=vio_marg_args),
    PriorCase("KBIG", lh.big, 3, 1, prior=kbig_prior),
    PriorCase("K258", k258, 2, 2, prior=lambda w: random_prior(w, [0, 2], 9700)),
]
CASE = {c.name: c for c in CASES}
_windows, _prior_windows, _refs = {}, {}, {}


def case_window(case):
    if case.window not in _windows:
        _windows[case.window] = case.build()
    return _windows[case.window]


def case_prior_window(case, oracle_lib=None):
    """The case's window under its prior: the oracle's marginalisation of its oldest key-frame, or the case's own."""
    if case.window not in _prior_windows:
        if oracle_lib is None:
            from oracle import oracle as oracle_lib
        w = case_window(case)
        w = with_oracle_prior(w, oracle_lib, case.marg) if case.prior is None else next_window(w, case.prior(w))
        kept = [int(l) for l, c in zip(w.dense_prior["lmk_index"], w.dense_prior["lmk_col"]) if c >= 0]
        n_long = len(set(kept) & set(lh.long_landmarks(w).tolist()))
        assert (len(kept), n_long) == (case.n_keep, case.n_keep_long), (case.name, len(kept), n_long)
        _prior_windows[case.window] = w
    return _prior_windows[case.window]


def case_options(case, iters=1):
    o = capi.gn_options(iters)
    for k, v in case.opts.items():
        setattr(o, k, v)
    return o


def reference(case, oracle_lib=None, fresh=False):
    """The 50-digit first step of the case's window under its prior: from the committed fixture, or computed (fresh)."""
    key = case.window
    if fresh:
        return sh.mp_first_step(case_prior_window(case, oracle_lib), case_options(case), oracle_lib=oracle_lib)
    if key not in _refs:
        w = case_window(case)
        z = np.load(GOLDEN)
        ref = {k: z[f"{key}/{k}"] for k in ("pose", "dv", "dba", "dbg", "lmk")}
        ref["model_cost_change"], ref["cost"] = float(z[f"{key}/model_cost_change"]), float(z[f"{key}/cost"])
        assert ref["pose"].shape == (w.n_kf, 6) and ref["lmk"].shape == (w.n_lmk, 3)
        _refs[key] = ref
    return _refs[key]


# (pose part, landmark part) of step_error(oracle float64 step, 50-digit step): measured by tests/test_long_prior_cpu.py, recorded
# 1.5 x the measured value rounded up (the test accepts a recorded value between 1 x and 4 x the measured one)
E_REF = {
    "KL65": (8.9e-14, 6.8e-14),
    "KMIX": (8.6e-14, 1.1e-12),
    "KL65_angular": (1.5e-13, 3.0e-13),
    "KL65_huber": (2.4e-14, 3.2e-14),
    "KVIO": (7.1e-15, 8.7e-13),
    "KBIG": (1.8e-12, 8.1e-13),
    "K258": (4.0e-13, 1.7e-14),
}


def bars(case):
    e = E_REF[case.window]
    return sh.TOL_FACTOR * max(e[0], sh.FLOOR), sh.TOL_FACTOR * max(e[1], sh.FLOOR)
