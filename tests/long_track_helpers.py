"""Windows with long tracks (landmarks of more than 64 observations: sadvio_amd/csrc/long_kernels.h) and their 50-digit first step:
the helper of tests/test_long_track_cpu.py, tests/test_long_plan_cpu.py and tests/test_gpu_long_tracks.py.

Every window is built once per process and never modified. The shapes are the smallest at which the long kernels can go wrong: 65
observations (one full round of a 64-lane group + 1), 128 and 129 (two rounds, two rounds + 1), long tracks at landmark index 0, in
the middle and last of a window whose other landmarks stay in the tiles, a constant long track, constant observers, the angular
factor, residuals on both sides of the Huber corner, IMU states, a second window of a batch, an observation that fails the
projection's tests, and a reduced system solved out of LDS whose band the long track fills.

E_REF[window] = step_error(oracle's float64 first step, 50-digit step), measured by tests/test_long_track_cpu.py and recorded here
1.5 x the measured value rounded up, as tests/step_helpers.py does; a device step passes at TOL_FACTOR x max(E_REF, FLOOR)."""
import dataclasses
import os

import numpy as np

import step_helpers as sh
from sadvio_amd import capi, synthetic

PIXEL, ANGULAR = capi.FACTOR_PIXEL, capi.FACTOR_ANGULAR
MAX_TILE_OBS = 64          # ba_types.h: MAX_LMK_OBS
MAX_LONG_OBS = 4096        # sadvio_ba.h: SADVIO_MAX_LONG_TRACK_OBS
MAX_LONG_KF = 512          # sadvio_ba.h: SADVIO_MAX_LONG_TRACK_KF
LONG_TEXT = "long track"   # every refusal that concerns long tracks says so
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "long_first_step_ref.npz")   # make_golden_long_first_step.py


def counts(w):
    return np.diff(w.lmk_obs_ptr)


def long_landmarks(w, long_min=MAX_TILE_OBS + 1):
    return np.flatnonzero(counts(w) >= long_min)


def l65(factor=PIXEL, **kw):
    """34 key-frames, 29 constant, 12 landmarks of 65 observations."""
    return synthetic.make_window(n_kf=34, n_lmk=12, obs_per_lmk=65, seed=9100, factor=factor, fixed=29, **kw)


def l128(n=128):
    """70 key-frames, 60 constant, 6 landmarks of 128 (129) observations."""
    return synthetic.make_window(n_kf=70, n_lmk=6, obs_per_lmk=n, seed=9200, fixed=60)


def _carry(dst, src, **extra):
    """_assemble keeps the key-frames: the constant flags, IMU states and factors of src come along."""
    for k in ("has_imu", "kf_vel", "kf_ba", "kf_bg", "imu_factors", "truth"):
        if getattr(src, k, None) is not None:
            setattr(dst, k, getattr(src, k))
    for k, v in extra.items():
        setattr(dst, k, v)
    return dst


def mix():
    """40 key-frames (34 constant): 60 landmarks of 5 observations, and landmarks of 66, 70 and 68 observations in front of landmark 0,
    in the middle and behind the last one; the middle one is constant."""
    import test_gpu_tile_packing as tp
    kw = dict(n_kf=40, seed=9300, fixed=34)
    pool = synthetic.make_window(n_lmk=600, obs_per_lmk=5, **kw)
    b = synthetic.make_window(n_lmk=24, obs_per_lmk=70, **kw)
    assert np.array_equal(pool.kf_T_f_w[pool.kf_const == 1], b.kf_T_f_w[b.kf_const == 1])   # same trajectory
    # the long tracks: the three of b seen most often from the free key-frames (a landmark's observations come oldest key-frame first)
    b_free = np.add.reduceat((b.kf_const[b.obs_kf] == 0).astype(int), b.lmk_obs_ptr[:-1])
    l0, l1, l2 = (int(v) for v in np.sort(np.argsort(-b_free, kind="stable")[:3]))
    # the 60 short tracks: those of the pool with the most observations from the 6 free key-frames (so that every free key-frame is well observed), in the pool's order
    n_free_obs = np.add.reduceat((pool.kf_const[pool.obs_kf] == 0).astype(int), pool.lmk_obs_ptr[:-1])
    short = np.sort(np.argsort(-n_free_obs, kind="stable")[:60])
    a = tp._assemble(pool, [(pool, int(l), None) for l in short])
    picks = [(b, l0, np.arange(4, 70))] + [(a, l, None) for l in range(30)] + [(b, l1, None)] + [(a, l, None) for l in range(30, 60)] + [(b, l2, np.arange(2, 70))]
    w = tp._assemble(a, picks)
    w.lmk_const = np.zeros(w.n_lmk, dtype=np.uint8)
    w.lmk_const[31] = 1
    assert long_landmarks(w).tolist() == [0, 31, 62] and w.n_lmk == 63
    return w


def mix_short():
    """MIX without its long tracks (the tiles of MIX must be the tiles of this window's landmarks)."""
    import test_gpu_tile_packing as tp
    w = mix()
    keep = [l for l in range(w.n_lmk) if counts(w)[l] <= MAX_TILE_OBS]
    s = tp._assemble(w, [(w, l, None) for l in keep])
    s.lmk_const = w.lmk_const[keep]
    return s


def l65_huber():
    """L65 from a small perturbation: part of the residuals inside the Huber corner, part beyond."""
    return l65(**sh.SMALL_PERTURB)


def vio_long():
    """A visual-inertial window (36 key-frames, 6 free, 15 states each) with one 66-observation landmark among 4-observation ones."""
    import test_gpu_tile_packing as tp
    from vio_helpers import make_vio_window
    a = make_vio_window(n_kf=36, n_lmk=72, obs_per_lmk=4, seed=9400, fixed=30)
    b = synthetic.make_window(n_kf=36, n_lmk=12, obs_per_lmk=66, seed=9400, fixed=30)
    assert np.array_equal(a.kf_T_f_w[a.kf_const == 1], b.kf_T_f_w[b.kf_const == 1])
    b_free = np.add.reduceat((b.kf_const[b.obs_kf] == 0).astype(int), b.lmk_obs_ptr[:-1])   # the one seen most often from the free key-frames
    w = _carry(tp._insert(a, {40: [(b, int(np.argmax(b_free)), None)]}), a)
    assert long_landmarks(w).tolist() == [40] and b_free.max() >= 6
    return w


INVALID_LMK = 3


def second_round_observation(w, l):
    """Caller's index of the observation at position 64 of landmark l's key-frame-sorted list (the library sorts stably by key-frame):
    the first observation of the second round of 64."""
    o = np.arange(w.lmk_obs_ptr[l], w.lmk_obs_ptr[l + 1])
    return int(o[np.argsort(w.obs_kf[o], kind="stable")][MAX_TILE_OBS])


def l65_invalid():
    """L65 with a third camera that looks backwards (camera 0 turned by 180 degrees about its y axis): every landmark lies behind it,
    so Camera::project's depth test fails there. The observation at position 64 of landmark 3 is taken by that camera: r = 0, Jacobian
    kept, in the second round."""
    w = l65()
    R = w.cam_T_s_f[0][:9].reshape(3, 3)
    t = w.cam_T_s_f[0][9:]
    F = np.diag([-1.0, 1.0, -1.0])
    back = np.concatenate([(F @ R).reshape(9), F @ t])
    w.cam_K = np.vstack([w.cam_K, w.cam_K[0]]); w.cam_T_s_f = np.vstack([w.cam_T_s_f, back]); w.cam_sigma = np.append(w.cam_sigma, w.cam_sigma[0])
    w.obs_cam = w.obs_cam.copy()
    w.obs_cam[second_round_observation(w, INVALID_LMK)] = 2
    return w


def big():
    """70 key-frames, 40 free (N_p = 240 > 174: solved out of LDS), narrow tracks everywhere and one landmark of 80 observations seen
    from the oldest to the newest free key-frame: the band is the whole matrix."""
    import test_gpu_tile_packing as tp
    kw = dict(n_kf=70, seed=9500, fixed=30, length=4.0)
    a = synthetic.make_window(n_lmk=70 * 12, obs_per_lmk=4, band=sh.SPREAD, **kw)
    b = synthetic.make_window(n_lmk=1, obs_per_lmk=140, **kw)
    assert np.array_equal(a.kf_T_f_w[a.kf_const == 1], b.kf_T_f_w[b.kf_const == 1])
    sel = np.arange(60, 140)      # (oldest view first) both cameras of the 40 newest key-frames: every free one
    w = tp._insert(a, {a.n_lmk // 2: [(b, 0, sel)]})
    assert counts(w).max() == 80
    return w


@dataclasses.dataclass
class LongCase:
    name: str
    build: object
    opts: dict = dataclasses.field(default_factory=dict)
    window: str = ""

    def __post_init__(self):
        self.window = self.window or self.name


CASES = [
    LongCase("L65", l65),
    LongCase("L128", lambda: l128(128)),
    LongCase("L129", lambda: l128(129)),
    LongCase("MIX", mix),
    LongCase("L65_angular", lambda: l65(ANGULAR)),
    LongCase("L65_huber", l65_huber, opts={"huber_a": sh.HUBER_A}),
    LongCase("VIO", vio_long),
    LongCase("L65_invalid", l65_invalid),
    LongCase("BIG", big),
]
CASE = {c.name: c for c in CASES}
_windows, _refs = {}, {}


def case_window(case):
    if case.window not in _windows:
        _windows[case.window] = case.build()
    return _windows[case.window]


def case_options(case, iters=1):
    o = capi.gn_options(iters)
    for k, v in case.opts.items():
        setattr(o, k, v)
    return o


def reference(case, oracle_lib=None, fresh=False):
    """The 50-digit first step of the case's window: read from the committed fixture (2 to 18 s of mpmath per window otherwise), or
    computed (fresh: the generator, and the CPU test that holds the fixture to a fresh computation)."""
    key = case.window
    if fresh:
        return sh.mp_first_step(case_window(case), case_options(case), oracle_lib=oracle_lib)
    if key not in _refs:
        w = case_window(case)
        z = np.load(GOLDEN)
        ref = {k: z[f"{key}/{k}"] for k in ("pose", "dv", "dba", "dbg", "lmk")}
        ref["model_cost_change"], ref["cost"] = float(z[f"{key}/model_cost_change"]), float(z[f"{key}/cost"])
        assert ref["pose"].shape == (w.n_kf, 6) and ref["lmk"].shape == (w.n_lmk, 3)
        _refs[key] = ref
    return _refs[key]


# (pose part, landmark part) of step_error(oracle float64 step, 50-digit step): measured by tests/test_long_track_cpu.py, recorded
# 1.5 x the measured value rounded up (the test accepts a recorded value between 1 x and 4 x the measured one)
E_REF = {
    "L65": (2.8e-13, 8.1e-13),
    "L128": (8.1e-13, 7.6e-14),
    "L129": (2.9e-12, 3.2e-13),
    "MIX": (2.0e-13, 6.5e-13),
    "L65_angular": (1.8e-13, 1.9e-13),
    "L65_huber": (2.5e-14, 4.4e-14),
    "VIO": (1.5e-14, 8.7e-13),
    "L65_invalid": (2.3e-13, 6.9e-13),
    "BIG": (1.6e-12, 8.1e-13),
}


def bars(case):
    e = E_REF[case.window]
    return sh.TOL_FACTOR * max(e[0], sh.FLOOR), sh.TOL_FACTOR * max(e[1], sh.FLOOR)
